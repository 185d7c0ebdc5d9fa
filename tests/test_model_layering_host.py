"""CPU tests of the model tier's layering: model/layers.py below everything, the trainable parts below the detectors, the
single-level families as siblings under SingleLevelDetector, one FC head, and constructors that create what they created before."""
import ast
import inspect
import os
import textwrap

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, 'tf_eager_object_detection_amd', 'model')
TRAINABLE = ('trainable_common', 'extractor_trainable', 'neck_trainable', 'rpn_trainable', 'vgg_trainable', 'c4_trainable')
LAYERED = ('fpn_detector', 'frcnn_detector', 'detector_base', 'layers') + TRAINABLE
SHARED_SINGLE_LEVEL = ('rpn', 'roi_head', '_dense', '_maps_of', '_per_image', '_prepare_per_image', '_per_image_to_head', 'rpn_trainable')


def _tree(name):
    return ast.parse(open(os.path.join(MODEL, name + '.py')).read())


def _siblings_imported(name):
    """the modules of model/ that model/<name>.py imports, read off its import statements"""
    found = set()
    for node in ast.walk(_tree(name)):
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            found |= {node.module.split('.')[0]} if node.module else {a.name for a in node.names}
        elif isinstance(node, (ast.Import, ast.ImportFrom)):
            full = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or '']
            found |= {f.split('.model.')[1].split('.')[0] for f in full if '.model.' in f}
    return found


def test_layers_is_the_bottom_and_no_trainable_part_imports_a_detector():
    assert _siblings_imported('layers') == set()
    pkg = 'tf_eager_object_detection_amd'
    for node in ast.walk(_tree('layers')):                      # (of the package: ops and derived only, however they are spelt)
        if isinstance(node, ast.ImportFrom) and node.level == 2:
            assert (node.module or [a.name for a in node.names][0]).split('.')[0] in ('ops', 'derived'), ast.dump(node)
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0, ast.dump(node)              # (level 1 = a sibling, level 3+ = outside the package)
            full = [node.module + '.' + a.name for a in node.names] if node.module == pkg else [node.module]
            assert all(f.split('.')[0] != pkg or f in (pkg + '.ops', pkg + '.derived') for f in full), ast.dump(node)
        elif isinstance(node, ast.Import):
            assert all(a.name.split('.')[0] != pkg or a.name in (pkg + '.ops', pkg + '.derived') for a in node.names), ast.dump(node)
    for name in TRAINABLE:
        got = _siblings_imported(name)
        assert not got & {'fpn_detector', 'frcnn_detector'}, (name, got)
        assert got <= {'layers', 'trainable_common', 'extractor_trainable', 'detector_base'}, (name, got)
        for node in ast.walk(_tree(name)):                      # (detector_base: for the float32 form's decorator only)
            if isinstance(node, ast.ImportFrom) and node.module == 'detector_base':
                assert [a.name for a in node.names] == ['_in_f32_form'], name
    assert _siblings_imported('detector_base') == {'layers'}
    # the detector files import the trainable parts, at module top
    assert {'extractor_trainable', 'neck_trainable', 'rpn_trainable', 'trainable_common'} <= _siblings_imported('fpn_detector')
    assert {'c4_trainable', 'vgg_trainable', 'rpn_trainable'} <= _siblings_imported('frcnn_detector')
    assert 'fpn_detector' not in _siblings_imported('frcnn_detector')


@pytest.mark.parametrize('name', LAYERED)
def test_no_import_inside_a_function(name):
    for fn in ast.walk(_tree(name)):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            inner = [n.lineno for n in ast.walk(fn) if isinstance(n, (ast.Import, ast.ImportFrom))]
            assert not inner, '%s.py: import inside %s() at line(s) %s' % (name, fn.name, inner)


def test_fpn_detector_defines_no_layer_builder_and_names_three_of_layers():
    from tf_eager_object_detection_amd.model import fpn_detector, layers
    assert fpn_detector.__all__ == ['ResNetFpnDetector', 'tf_legacy_resize_bilinear']
    assert fpn_detector.tf_legacy_resize_bilinear is layers.tf_legacy_resize_bilinear
    src = inspect.getsource(fpn_detector)
    for name in ('_route_1x1', '_mfma_ok', '_patch_gemm', '_PATCH_BYTES_MAX', '_FUSED_TAIL_MIN_SLABS', '_BN_EPS'):
        assert not hasattr(fpn_detector, name) and name not in src, name
    # (besides the public resize, two builders stay importable from fpn_detector: the test files of the commit before
    # model/layers.py take them from there and are run against this package; both are layers' own objects)
    assert fpn_detector._Block is layers._Block and fpn_detector._conv_relu_pool is layers._conv_relu_pool
    defined = [n.name for n in _tree('fpn_detector').body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    assert defined == ['ResNetFpnDetector']


def test_single_level_families_are_siblings():
    from tf_eager_object_detection_amd.model.detector_base import Detector
    from tf_eager_object_detection_amd.model.frcnn_detector import ResNetC4Detector, SingleLevelDetector, Vgg16Detector
    assert not issubclass(Vgg16Detector, ResNetC4Detector) and not issubclass(ResNetC4Detector, Vgg16Detector)
    for cls in (ResNetC4Detector, Vgg16Detector):
        assert issubclass(cls, SingleLevelDetector) and cls.__bases__ == (SingleLevelDetector,)
        for name in SHARED_SINGLE_LEVEL + ('_step_batch_class', '_hot_path_class'):
            assert inspect.getattr_static(cls, name) is SingleLevelDetector.__dict__[name], (cls.__name__, name)
        for name in ('prepare', 'forward', 'im_detect', 'capture'):
            assert getattr(cls, name) is Detector.__dict__[name], (cls.__name__, name)
        for name in ('__init__', 'features', 'head_activation', 'extractor_trainable', 'roi_head_trainable'):
            assert name in cls.__dict__ and name not in SingleLevelDetector.__dict__, (cls.__name__, name)
    assert SingleLevelDetector.__bases__ == (Detector,)
    assert 'nn.Module.__init__' not in inspect.getsource(inspect.getmodule(Vgg16Detector))


def _delegates_to(method, target):
    """the method's body, after its docstring, is one `return <target>(self, ...)`"""
    fn = ast.parse(textwrap.dedent(inspect.getsource(method))).body[0]
    body = fn.body[1:] if ast.get_docstring(fn) is not None else fn.body
    if len(body) != 1 or not isinstance(body[0], ast.Return) or not isinstance(body[0].value, ast.Call):
        return False
    call = body[0].value
    name = call.func.id if isinstance(call.func, ast.Name) else getattr(call.func, 'attr', None)
    return name == target and isinstance(call.args[0], ast.Name) and call.args[0].id == 'self'


def test_one_fc_head_and_one_pattern_for_the_trainable_parts():
    from tf_eager_object_detection_amd.model import fpn_detector, frcnn_detector, layers, trainable_common, vgg_trainable
    fpn, c4, vgg = fpn_detector.ResNetFpnDetector, frcnn_detector.ResNetC4Detector, frcnn_detector.Vgg16Detector
    for mod in (fpn_detector, frcnn_detector):
        assert mod.fc_head_activation is layers.fc_head_activation and mod.fc_head_trainable is trainable_common.fc_head_trainable
    assert vgg_trainable.roi_head_trainable is trainable_common.fc_head_trainable
    for cls in (fpn, vgg):
        assert _delegates_to(cls.head_activation, 'fc_head_activation'), cls.__name__
        assert _delegates_to(cls.roi_head_trainable, 'fc_head_trainable'), cls.__name__
    sig = inspect.signature(trainable_common.fc_head_trainable).parameters
    assert [(k, sig[k].default) for k in ('keep_prob', 'seed', 'image_id')] == [('keep_prob', 1.0), ('seed', 0), ('image_id', 0)]
    # every trainable part of the three detectors: decorated (functools.wraps leaves __wrapped__), documented, one delegating line
    for cls, names in ((fpn, ('extractor_trainable', 'neck_trainable', 'rpn_trainable', 'roi_head_trainable')),
                       (c4, ('extractor_trainable', 'roi_head_trainable')), (vgg, ('extractor_trainable', 'roi_head_trainable'))):
        for name in names:
            m = cls.__dict__[name]
            target = 'fc_head_trainable' if name == 'roi_head_trainable' and cls is not c4 else name
            assert hasattr(m, '__wrapped__') and m.__doc__ and _delegates_to(m, target), (cls.__name__, name)


def test_vgg16_has_nothing_of_the_c4_network():
    from tf_eager_object_detection_amd.model import c4_trainable
    from tf_eager_object_detection_amd.model.frcnn_detector import Vgg16Detector
    assert not hasattr(c4_trainable, 'C4TrainableParts')
    det = Vgg16Detector(21, (64, 64), 10)
    for name in ('conv1', 'conv2', 'conv3', 'conv4', 'conv5', '_roi_chunk'):
        assert not hasattr(det, name), name
    assert not any(str(getattr(f, '__module__', '')).endswith('c4_trainable') for k in Vgg16Detector.__mro__ for f in vars(k).values())
    with pytest.raises(AttributeError):
        c4_trainable.extractor_trainable(det, torch.zeros(1, 64, 64, 3))
    with pytest.raises(AttributeError):
        c4_trainable.roi_head_trainable(det, torch.zeros(2, 7, 7, 1024))


# the parameters of the three detectors in named_parameters() order on the commit before model/layers.py existed: each entry a
# module with its weight and its bias
_RESNET50_C1_C4 = '''conv1 conv2.0.short conv2.0.c1 conv2.0.c2 conv2.0.c3 conv2.1.c1 conv2.1.c2 conv2.1.c3 conv2.2.c1 conv2.2.c2 conv2.2.c3
conv3.0.short conv3.0.c1 conv3.0.c2 conv3.0.c3 conv3.1.c1 conv3.1.c2 conv3.1.c3 conv3.2.c1 conv3.2.c2 conv3.2.c3
conv3.3.c1 conv3.3.c2 conv3.3.c3 conv4.0.short conv4.0.c1 conv4.0.c2 conv4.0.c3 conv4.1.c1 conv4.1.c2 conv4.1.c3
conv4.2.c1 conv4.2.c2 conv4.2.c3 conv4.3.c1 conv4.3.c2 conv4.3.c3 conv4.4.c1 conv4.4.c2 conv4.4.c3 conv4.5.c1 conv4.5.c2
conv4.5.c3 '''
_RESNET50_C5 = 'conv5.0.short conv5.0.c1 conv5.0.c2 conv5.0.c3 conv5.1.c1 conv5.1.c2 conv5.1.c3 conv5.2.c1 conv5.2.c2 conv5.2.c3 '
PARAMETERS = {
    'fpn': _RESNET50_C1_C4 + _RESNET50_C5 + 'p5 l4 l3 l2 s4 s3 s2 rpn_conv rpn_score rpn_bbox fc1 fc2 score bbox',
    'c4': _RESNET50_C1_C4 + 'rpn_conv rpn_score rpn_bbox ' + _RESNET50_C5 + 'score bbox',
    'vgg16': 'convs.0 convs.1 convs.2 convs.3 convs.4 convs.5 convs.6 convs.7 convs.8 convs.9 convs.10 convs.11 convs.12 rpn_conv '
             'rpn_score rpn_bbox fc1 fc2 score bbox',
}


@pytest.mark.parametrize('family', sorted(PARAMETERS))
def test_construction_gives_the_parameter_names_of_before(family):
    from tf_eager_object_detection_amd.model.fpn_detector import ResNetFpnDetector
    from tf_eager_object_detection_amd.model.frcnn_detector import ResNetC4Detector, Vgg16Detector
    torch.manual_seed(1)
    det = {'fpn': lambda: ResNetFpnDetector(50), 'c4': lambda: ResNetC4Detector(50), 'vgg16': Vgg16Detector}[family]()
    want = [m + s for m in PARAMETERS[family].split() for s in ('.weight', '.bias')]
    assert len(want) == {'fpn': 134, 'c4': 116, 'vgg16': 40}[family]
    assert [n for n, _ in det.named_parameters()] == want
    assert (det.dtype, det.f32_form, det.grad_form, det.num_classes) == (torch.float32, 'exact', 'exact', 21)
    assert det.image_shape == {'fpn': (800, 1333), 'c4': (800, 1333), 'vgg16': (600, 800)}[family] and det.A == (3 if family == 'fpn' else 9)


def test_line_budget():
    """non-blank, non-comment lines of the ten files: 1422 over the nine that existed before model/layers.py"""
    total = 0
    for name in LAYERED:
        lines = open(os.path.join(MODEL, name + '.py')).read().splitlines()
        total += sum(1 for ln in lines if ln.strip() and not ln.strip().startswith('#'))
    assert total < 1422, total
