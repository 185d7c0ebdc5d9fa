"""The Dense backward without a GPU: the float64 statement (tests/dense_grad_np.py) against torch.autograd, the refusal rules of
odet_dense_dgrad_f32 / odet_dense_wgrad_f32 through the built library (each returns before any HIP call), and the Python
fronts' argument errors on CPU tensors."""
import numpy as np
import pytest
import torch

import dense_grad_np as dg


def _layer(rng, rows, cin, cout):
    x = rng.integers(-3, 4, (rows, cin)).astype(np.float64)
    w = rng.integers(-2, 3, (cout, cin)).astype(np.float64)
    b = rng.integers(-2, 3, (cout,)).astype(np.float64)
    return x, w, b


def test_statement_equals_torch_autograd_of_a_relu_layer():
    """dx, dw, db of relu(x @ w.T + b) in float64; integer data makes many pre-activations EXACTLY zero, whose gradient must be
    zero (y > 0 is strict), and some negative"""
    rng = np.random.default_rng(0)
    x, w, b = _layer(rng, 9, 6, 5)
    dy = rng.standard_normal((9, 5))
    tx, tw, tb = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    pre = tx @ tw.T + tb
    y = torch.relu(pre)
    y.backward(torch.tensor(dy))
    pre = pre.detach().numpy()
    assert (pre == 0).sum() >= 2 and (pre < 0).sum() >= 2 and (pre > 0).sum() >= 2
    yn = y.detach().numpy()
    np.testing.assert_array_equal(dg.masked_dy(dy, yn)[pre == 0], 0.0)
    dw, db = dg.wgrad(dy, x, yn)
    np.testing.assert_allclose(dg.dgrad(dy, w, yn), tx.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dw, tw.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(db, tb.grad.numpy(), rtol=1e-13, atol=1e-13)
    # without a ReLU: no mask
    tx2, tw2, tb2 = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    (tx2 @ tw2.T + tb2).backward(torch.tensor(dy))
    dw, db = dg.wgrad(dy, x)
    np.testing.assert_allclose(dg.dgrad(dy, w), tx2.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dw, tw2.grad.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(db, tb2.grad.numpy(), rtol=1e-13, atol=1e-13)
    # a NaN under a closed gate does not pass (a select, not a product)
    bad = dy.copy()
    bad[pre <= 0] = np.nan
    assert np.isfinite(dg.dgrad(bad, w, yn)).all()


def test_statement_two_layer_chain_with_x_relu():
    """h = relu(x w1^T + b1), y = relu(h w2^T + b2): layer 2's dgrad with x_relu = h IS layer 1's dz, so layer 1's wgrad on it
    needs no mask of its own"""
    rng = np.random.default_rng(1)
    x, w1, b1 = _layer(rng, 7, 6, 8)
    _, w2, b2 = _layer(rng, 7, 8, 4)
    dy = rng.standard_normal((7, 4))
    t = [torch.tensor(a, requires_grad=True) for a in (x, w1, b1, w2, b2)]
    h = torch.relu(t[0] @ t[1].T + t[2])
    y = torch.relu(h @ t[3].T + t[4])
    y.backward(torch.tensor(dy))
    hn, yn = h.detach().numpy(), y.detach().numpy()
    assert (hn == 0).any() and (yn == 0).any()
    dw2, db2 = dg.wgrad(dy, hn, yn)
    dh = dg.dgrad(dy, w2, yn, x_relu=hn)
    dw1, db1 = dg.wgrad(dh, x)
    dw1m, db1m = dg.wgrad(dg.dgrad(dy, w2, yn), x, hn)              # (the other reading: the mask in layer 1's staging)
    for got, want in ((dw2, t[3].grad), (db2, t[4].grad), (dw1, t[1].grad), (db1, t[2].grad), (dw1m, t[1].grad), (db1m, t[2].grad),
                      (dg.dgrad(dh, w1), t[0].grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-13, atol=1e-13)


# ---- the refusal rules, through the built library: pointer-VALUED integers nothing dereferences (the float32-form table of
# test_host_logic.py does the same); every row returns before any HIP call, so this runs without a GPU
_NAMES = {
    'dgrad': ('dy', 'w', 'y_relu', 'x_relu', 'dx', 'rows', 'cin', 'cout', 'ws', 'ws_bytes', 'stream'),
    'wgrad': ('dy', 'x', 'y_relu', 'dw', 'db', 'rows', 'cin', 'cout', 'ws', 'ws_bytes', 'stream'),
}
_GOOD = dict(dy=0x10000, w=0x20000, x=0x20000, y_relu=0x30000, x_relu=0x40000, dx=0x50000, dw=0x50000, db=0x60000, rows=5, cin=64,
             cout=64, ws=None, ws_bytes=0, stream=None)
_SHAPES = [('cin 48', {'cin': 48}), ('cin 32', {'cin': 32}), ('cin 0', {'cin': 0}), ('cin -64', {'cin': -64}), ('cout 96', {'cout': 96}),
           ('cout 0', {'cout': 0}), ('rows 0', {'rows': 0}), ('rows -1', {'rows': -1})]
_ROWS = {
    'dgrad': [('null ' + n, {n: None}) for n in ('dy', 'w', 'dx')] + _SHAPES
    + [('misaligned ' + n, {n: _GOOD[n] + 4}) for n in ('dy', 'w', 'y_relu', 'x_relu', 'dx')],
    'wgrad': [('null ' + n, {n: None}) for n in ('dy', 'x', 'dw')] + _SHAPES
    + [('misaligned ' + n, {n: _GOOD[n] + 4}) for n in ('dy', 'x', 'y_relu', 'dw')] + [('misaligned db', {'db': _GOOD['db'] + 2})],
}
# shapes whose launch splits its contraction (few tiles, contraction >= 256): the head's fc2 dgrad, the final layer's wgrad
_SPLIT = {'dgrad': dict(rows=256, cin=1024, cout=1024), 'wgrad': dict(rows=256, cin=1024, cout=128)}


@pytest.mark.parametrize('kind', ['dgrad', 'wgrad'])
def test_entry_points_refuse_bad_arguments_before_any_device_call(kind):
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    fn = getattr(L, 'odet_dense_%s_f32' % kind)
    for label, bad in _ROWS[kind]:
        args = dict(_GOOD)
        args.update(bad)
        rc = fn(*[args[n] for n in _NAMES[kind]])
        msg = L.odet_last_error()
        print('%s: %s -> %d %r' % (kind, label, rc, msg))
        assert rc == -1, '%s: %s returned %d: %r' % (kind, label, rc, msg)                          # ODET_E_INVALID
        assert msg.startswith(b'odet_dense_%s_f32' % kind.encode()) and b' failed: ' not in msg, msg  # (no HIP call was made)
    # a workspace that is missing, too small or misaligned where the launch needs one
    s = _SPLIT[kind]
    need = L.odet_dense_grad_workspace_bytes(1 if kind == 'wgrad' else 0, s['rows'], s['cin'], s['cout'])
    assert need >= 2 * 4 * s['cin'] * (s['cout'] if kind == 'wgrad' else s['rows'])
    for label, bad, want in (('no workspace', dict(ws=None, ws_bytes=need), -2), ('workspace one byte short', dict(ws=0x100000, ws_bytes=need - 1), -2),
                             ('workspace of 0 bytes', dict(ws=0x100000, ws_bytes=0), -2), ('misaligned workspace', dict(ws=0x100004, ws_bytes=need), -1)):
        args = dict(_GOOD, **s)
        args.update(bad)
        rc = fn(*[args[n] for n in _NAMES[kind]])
        msg = L.odet_last_error()
        print('%s: %s -> %d %r' % (kind, label, rc, msg))
        assert rc == want and b' failed: ' not in msg, (label, rc, msg)


def test_workspace_query_is_a_function_of_the_shape():
    from tf_eager_object_detection_amd import _lib
    L = _lib.lib()
    q = L.odet_dense_grad_workspace_bytes
    # the exactness grid of the GPU tests takes no split (contraction < 256) ...
    for rows in (1, 2, 3, 5, 17, 64, 130):
        for cin in (64, 96, 160):
            for cout in (64, 192):
                assert q(0, rows, cin, cout) == 0 and q(1, rows, cin, cout) == 0
    # ... the head's layers at rows = 256 do where the tiles are few: fc2's dgrad in 4 parts, the final layer's wgrad in 4
    assert q(0, 256, 1024, 1024) == 4 * 256 * 1024 * 4
    assert q(1, 256, 1024, 1024) == 0 and q(1, 256, 12544, 1024) == 0
    assert q(1, 256, 1024, 128) == 4 * 128 * 1024 * 4
    assert q(0, 37, 1024, 128) == 0 and q(1, 37, 1024, 128) == 0
    assert q(1, 0, 64, 64) == 0


def test_python_fronts_refuse_on_cpu_tensors():
    from tf_eager_object_detection_amd import ops
    dy, w, x = torch.zeros(4, 64), torch.zeros(64, 64), torch.zeros(4, 64)
    for call in (lambda **k: ops.dense_dgrad(k.get('dy', dy), k.get('w', w), k.get('y')),
                 lambda **k: ops.dense_wgrad(k.get('dy', dy), k.get('w', x), k.get('y'))):
        with pytest.raises(ValueError, match='float32'):
            call(dy=dy.half())
        with pytest.raises(ValueError, match='float32'):
            call(w=w.half())
        with pytest.raises(ValueError, match='float32'):
            call(y=dy.double())
        for form in ('x3', 'x2'):
            with ops.f32_form(form):
                with pytest.raises(ValueError, match="only under f32_form 'exact'"):
                    call()
        with pytest.raises(ValueError, match='contiguous'):
            call(dy=torch.zeros(64, 4).t())
        with pytest.raises(ValueError, match='contiguous'):
            call(w=torch.zeros(64, 64).t())
        with pytest.raises(ValueError, match='contiguous'):
            call(y=torch.zeros(64, 4).t())
        with pytest.raises(ValueError, match='GPU'):                 # (and no CPU path behind the checks)
            call()
    with ops.f32_form('x3'):
        with pytest.raises(ValueError, match="only under f32_form 'exact'"):
            ops.dense_trainable(x, w, None)
    with pytest.raises(ValueError, match='float32'):
        ops.dense_trainable(x.half(), w.half(), None)


def test_caller_model_refuses_train_roi_head_outside_the_exact_float32_form():
    import inspect
    from tf_eager_object_detection_amd.model.base_fpn_model import BaseFPN, ResnetV1Fpn
    for cls in (BaseFPN, ResnetV1Fpn):
        assert inspect.signature(cls.__init__).parameters['train_roi_head'].default is False
    with pytest.raises(ValueError, match='train_roi_head'):
        ResnetV1Fpn(depth=50, train_roi_head=True, f32_form='x3', device='cpu')
    with pytest.raises(ValueError, match='train_roi_head'):
        ResnetV1Fpn(depth=50, train_roi_head=True, dtype=torch.float16, device='cpu')
