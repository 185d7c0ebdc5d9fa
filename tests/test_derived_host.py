"""derived.py on CPU tensors: the one validity rule of every weight-derived tensor, with a builder that counts its calls."""
import torch
import torch.nn as nn

from tf_eager_object_detection_amd.derived import derived, invalidate

ATTR = '_odet_derived'


class Doubler:
    """build(*sources) -> the first source times two; counts its calls"""

    def __init__(self):
        self.calls = 0

    def __call__(self, *sources):
        self.calls += 1
        return sources[0].detach().float() * 2


def test_same_sources_build_once_and_an_in_place_update_rebuilds():
    w, build = torch.randn(4, 3), Doubler()
    a = derived(w, 'd', (w,), build)
    assert derived(w, 'd', (w,), build) is a and build.calls == 1
    with torch.no_grad():
        w.mul_(2)
    b = derived(w, 'd', (w,), build)
    assert build.calls == 2 and torch.equal(b, w * 2)
    assert derived(w, 'd', (w,), build) is b and build.calls == 2
    # two names on one holder are two entries of the holder's one dict
    other = Doubler()
    derived(w, 'e', (w,), other)
    assert derived(w, 'd', (w,), build) is b and (build.calls, other.calls) == (2, 1)
    assert set(w.__dict__[ATTR]) == {'d', 'e'}


def test_a_data_write_is_not_seen_until_invalidate():
    w, build = nn.Parameter(torch.randn(4, 3)), Doubler()
    a = derived(w, 'd', (w,), build)
    w.data.mul_(2)                                       # (no version bump: documented, needs invalidate / prepare())
    assert derived(w, 'd', (w,), build) is a and build.calls == 1
    invalidate(w)
    assert ATTR not in w.__dict__
    assert torch.equal(derived(w, 'd', (w,), build), w.detach() * 2) and build.calls == 2


def test_module_conversion_rebuilds_and_nothing_reaches_the_state_dict():
    m, build = nn.Linear(3, 4), Doubler()
    w = m.weight
    derived(m, 'd', (m.weight, m.bias), build)
    derived(m, 'd', (m.weight, m.bias), build)
    assert build.calls == 1
    assert set(m.state_dict()) == {'weight', 'bias'} and ATTR in m.__dict__
    m.to(torch.float16)
    assert m.weight is w and w.dtype == torch.float16         # the parameter object is kept: dtype and pointer changed
    derived(m, 'd', (m.weight, m.bias), build)
    assert build.calls == 2
    m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
    derived(m, 'd', (m.weight, m.bias), build)
    assert build.calls == 3
    assert set(m.state_dict()) == {'weight', 'bias'}


def test_another_object_at_the_same_address_and_version_misses():
    m, build = nn.Linear(3, 4), Doubler()
    w = m.weight
    derived(m, 'd', (w,), build)
    b = w.detach()
    assert b is not w and b.data_ptr() == w.data_ptr() and b._version == w._version and b.stride() == w.stride()
    derived(m, 'd', (b,), build)
    assert build.calls == 2
    # the entry keeps its source alive, so its address cannot be handed out again while the entry exists
    assert m.__dict__[ATTR]['d'][0][0] is b


def test_inference_tensors_are_built_every_time_and_store_nothing():
    build = Doubler()
    with torch.inference_mode():
        w = torch.randn(4, 3)
    m = nn.Linear(3, 4)
    for holder in (w, m):
        before = build.calls
        derived(holder, 'd', (w,), build)
        derived(holder, 'd', (w,), build)
        assert build.calls == before + 2 and ATTR not in holder.__dict__


def test_a_builder_may_return_a_tuple():
    m = nn.Linear(3, 4)
    w, b = derived(m, 'pair', (m.weight, m.bias), lambda w, b: (w.detach() + 1, b.detach() + 1))
    w2, b2 = derived(m, 'pair', (m.weight, m.bias), lambda w, b: (w.detach() + 1, b.detach() + 1))
    assert w2 is w and b2 is b


def test_invalidate_module_reaches_sub_modules_parameters_and_chained_entries():
    net = nn.Sequential(nn.Linear(3, 4), nn.Sequential(nn.Linear(4, 4)))
    net.register_buffer('scale', torch.ones(3))
    inner, build = net[1][0], Doubler()
    cat = derived(inner, 'cat', (inner.weight, inner.bias), build)             # a module entry ...
    planes = derived(cat, 'planes', (cat,), build)                              # ... whose value holds an entry of its own
    derived(inner.weight, 'planes', (inner.weight,), build)                     # a parameter's entry
    derived(net.scale, 'planes', (net.scale,), build)                           # a buffer's entry
    derived(net, 'top', (net[0].weight,), build)
    assert build.calls == 5
    assert derived(derived(inner, 'cat', (inner.weight, inner.bias), build), 'planes', (cat,), build) is planes
    assert build.calls == 5
    invalidate(net)
    for holder in (net, inner, inner.weight, net.scale):
        assert ATTR not in holder.__dict__
    cat2 = derived(inner, 'cat', (inner.weight, inner.bias), build)
    assert cat2 is not cat and ATTR not in cat2.__dict__                        # the chained entry went with its holder
    derived(cat2, 'planes', (cat2,), build)
    derived(inner.weight, 'planes', (inner.weight,), build)
    derived(net.scale, 'planes', (net.scale,), build)
    derived(net, 'top', (net[0].weight,), build)
    assert build.calls == 10
