"""The ONE precedence of the float32 backward ops' Python fronts (ops._grad_operands / ops._grad_on_gpu): dtype -> f32 form -> rank
and contiguity -> the front's own shape rules -> GPU.  Every front is fed two faults at once and must report the earlier one; the
operands are the smallest legal CPU tensors, so everything stops at the last rule ("must be a GPU tensor") at the latest and no
GPU is needed."""
import pytest
import torch


def _ops():
    from tf_eager_object_detection_amd import ops
    return ops


def _strided(t):
    """t's values and shape, not contiguous"""
    return t.unsqueeze(-1).repeat(*([1] * t.dim()), 2)[..., 0]


ROWS, CIN, COUT = 4, 64, 64
F = torch.zeros


def _dense_dgrad(t):
    return _ops().dense_dgrad(t['dy'], t['weight'])


def _dense_wgrad(t):
    return _ops().dense_wgrad(t['dy'], t['x'])


def _conv_wgrad(t):
    return _ops().conv3x3_wgrad_f32_levels([t['x']], [t['dy']])


def _conv_dgrad(t):
    return _ops().conv3x3_dgrad_f32_levels([t['dz']], t['weight'])


def _topdown(t):
    return _ops().fpn_topdown_backward(t['fine'], (1, 2), base=t['base'])


def _gather(t):
    return _ops().stride_gather(t['x'], t.get('stride', 2))


def _join(t):
    return _ops().block_input_grad(t['d1'], dy=t['dy'], y=t['y'])


def _pool(t):
    return _ops().relu_maxpool2_backward(t['z'], t['bias'], t['dpool'])


def _dropout(t):
    return _ops().dropout(t['x'], t.get('keep_prob', 0.5), 0, 0, 6)


def _dropout_backward(t):
    return _ops().dropout_backward(t['dy'], t.get('keep_prob', 0.5), 0, 0, 6)


# name -> (call, valid CPU operands, the operand that takes the dtype / contiguity fault, a shape fault, its message)
FRONTS = {
    'dense_dgrad': (_dense_dgrad, lambda: dict(dy=F(ROWS, COUT), weight=F(COUT, CIN)), 'dy',
                    dict(weight=F(COUT, 48)), 'multiple of 32'),
    'dense_wgrad': (_dense_wgrad, lambda: dict(dy=F(ROWS, COUT), x=F(ROWS, CIN)), 'x',
                    dict(x=F(ROWS + 1, CIN)), 'does not go with'),
    'conv3x3_wgrad_f32_levels': (_conv_wgrad, lambda: dict(x=F(1, 2, 3, CIN), dy=F(1, 2, 3, COUT)), 'x',
                                 dict(dy=F(1, 2, 3, 32)), 'multiple of 64'),
    'conv3x3_dgrad_f32_levels': (_conv_dgrad, lambda: dict(dz=F(1, 2, 3, COUT), weight=F(COUT, CIN, 3, 3)), 'dz',
                                 dict(weight=F(COUT, 32, 3, 3)), 'multiple of 64'),
    'fpn_topdown_backward': (_topdown, lambda: dict(fine=F(1, 2, 3, 4), base=F(1, 1, 2, 4)), 'fine',
                             dict(base=F(1, 2, 2, 4)), 'does not go with'),
    'stride_gather': (_gather, lambda: dict(x=F(1, 2, 3, 4)), 'x', dict(stride=3), 'stride must be 1 or 2'),
    'block_input_grad': (_join, lambda: dict(d1=F(1, 2, 3, 4), dy=F(1, 2, 3, 4), y=F(1, 2, 3, 4)), 'd1',
                         dict(y=F(1, 2, 2, 4)), 'does not go with'),
    'relu_maxpool2_backward': (_pool, lambda: dict(z=F(1, 2, 3, 4), bias=F(4), dpool=F(1, 1, 2, 4)), 'z',
                               dict(dpool=F(1, 2, 2, 4)), 'does not go with'),
    'dropout': (_dropout, lambda: dict(x=F(2, 3)), 'x', dict(keep_prob=1.5), 'keep_prob'),
    'dropout_backward': (_dropout_backward, lambda: dict(dy=F(2, 3)), 'dy', dict(keep_prob=0.0), 'keep_prob'),
}


@pytest.mark.parametrize('front', list(FRONTS))
def test_backward_fronts_report_the_first_fault_in_one_order(front):
    ops = _ops()
    call, make, first, bad_shape, shape_message = FRONTS[front]

    def refuses(operands, match, form='exact'):
        with ops.f32_form(form):
            with pytest.raises(ValueError, match=match) as e:
                call(operands)
        assert str(e.value).startswith(front + ': '), e.value

    t = make()
    refuses(dict(t, **{first: t[first].half()}), 'must be a float32 tensor', form='x3')        # dtype before the form
    refuses(dict(t, **{first: _strided(t[first])}), "only under f32_form 'exact'", form='x3')  # the form before contiguity
    refuses(dict(t, **{first: _strided(t[first])}), 'contiguous')                              # contiguity before the device
    refuses(dict(t, **bad_shape), shape_message)                                               # the shape rules before the device
    refuses(t, 'must be a GPU tensor')                                                         # and no CPU path behind the checks


def test_the_fronts_share_one_message_template():
    """the nouns differ, the sentences do not"""
    nouns = set()
    for front, (call, make, first, _, _) in FRONTS.items():
        t = make()
        with pytest.raises(ValueError) as e:
            call(dict(t, **{first: t[first].double()}))
        msg = str(e.value)
        assert msg.startswith(front + ': ') and ' must be a float32 tensor (the ' in msg, msg
        assert msg.endswith(' has no float16 form), got torch.float64'), msg
        nouns.add(msg.split('(the ')[1].split(' has no')[0])
    assert nouns == {'Dense backward', 'convolution backward', 'neck backward', 'bottleneck backward', 'max-pooling backward',
                     'dropout'}
