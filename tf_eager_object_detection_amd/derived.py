"""Tensors derived from weights (limb planes, packed / padded / concatenated weights), kept ON the object they belong to.

ONE rule decides whether a derived value is still valid: every source is the same tensor OBJECT as at build time and has the
same (data_ptr, _version, dtype, device, shape, stride).  In-place operations through the tensor, load_state_dict(), an
optimizer step and Module.to() change one of these, so the value rebuilds by itself at its next use; a write that leaves all of
them alone (`.data` writes, set_() to an equal layout) needs `invalidate` (the detectors' prepare() calls it).

Nothing is stored globally: the entries of a holder live in holder.__dict__['_odet_derived'] -- exactly as long as the holder,
never in a state_dict(), and (for a module) past Module.__setattr__.  An entry keeps its sources alive, so an address cannot be
recycled under it.  A derived tensor may itself be a holder (the limb planes of a padded weight live on the padded weight): it
is reachable only through its holder's entries and goes with them.
"""
import torch

_ATTR = '_odet_derived'


def _state(t):
    # (id: the entry keeps `t` alive, so an equal id IS the same object)
    return (id(t), t.data_ptr(), t._version, t.dtype, t.device, t.size(), t.stride())


def derived(holder, name, sources, build):
    """build(*sources), cached under `name` on `holder` (an nn.Module or a tensor) until a source changes (the module
    docstring's rule).  `sources`: a tuple of STABLE tensor objects -- parameters, or derived values; a caller that passes a
    fresh temporary every time pays the build every time (correct, slow).  A source without a version counter (inference
    tensors: torch raises on ._version) is never cached: build runs on every call."""
    try:
        states = [_state(t) for t in sources]
    except RuntimeError:
        return build(*sources)
    entries = holder.__dict__.get(_ATTR)
    hit = entries.get(name) if entries is not None else None
    if hit is not None and hit[1] == states:
        return hit[2]
    value = build(*sources)
    if entries is None:
        entries = holder.__dict__[_ATTR] = {}
    entries[name] = (sources, states, value)
    return value


def invalidate(obj):
    """drops every derived value of a tensor, or of every sub-module, parameter and buffer of an nn.Module (and with them the
    values derived from those): call after writing weights in a way the rule cannot see"""
    holders = [obj]
    if isinstance(obj, torch.nn.Module):
        holders = [*obj.modules(), *obj.parameters(), *obj.buffers()]
    for h in holders:
        h.__dict__.pop(_ATTR, None)
