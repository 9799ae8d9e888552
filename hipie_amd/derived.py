"""The one cache for values derived from parameters: HL8 / f8x copies of weights, folded or concatenated projections, transposed MLP
heads, resized position tables.  (Caches keyed on shapes alone -- geo_cached, window_row_maps, level_tensors -- are a different thing.)"""
import weakref

import torch


def stamp(params):
    """what identifies the contents of ``params`` (tensors or None): per tensor (data_ptr, _version, dtype, device, shape).  In-place
    updates move _version; load_state_dict, .to(), ``p.data = ...`` move _version, data_ptr or dtype."""
    return tuple([None if p is None else (p.data_ptr(), p._version, p.dtype, p.device, p.shape) for p in params])


def _gone():          # stands in for the weak reference of a None entry: a dead reference also answers None, and then the stamps differ
    return None


def derived(owner, name, params, build, extra=(), keep=1):
    """``build()`` (run under no_grad), cached on ``owner`` -- a module, a tensor, anything with a __dict__ -- under ``name``; rebuilt when
    stamp(params) or ``extra`` (what is not a tensor: token grid, dtype, format tag) changes.  The entry holds the parameters weakly
    and hits only while they are the SAME tensor objects, so a stamp re-used by a new tensor at a freed address misses.  ``keep``: how
    many values of ``extra`` stay alive side by side under one name (oldest built goes first); 1 = rebuild whenever ``extra`` changes."""
    slot = owner.__dict__.setdefault("_derived", {}).setdefault(name, {})           # extra -> (weak references, stamp, value)
    e = slot.get(extra)
    st = stamp(params)
    if e is not None and e[1] == st and all([r() is p for r, p in zip(e[0], params)]):
        return e[2]
    with torch.no_grad():
        value = build()
    slot.pop(extra, None)
    while len(slot) >= keep:
        del slot[next(iter(slot))]
    slot[extra] = (tuple(_gone if p is None else weakref.ref(p) for p in params), st, value)
    return value


def clear(module):
    """drop every derived value cached on ``module`` and its sub-modules"""
    for m in module.modules():
        m.__dict__.pop("_derived", None)
