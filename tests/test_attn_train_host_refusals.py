"""Host-side refusals of the GLOBAL fused training attention (hipie_attn_train_forward / _backward, csrc/attn_train.hip); the windowed
entries' are in test_attn_train_win_cpu.py.  Every call violates one condition of the entry check, so it is refused on the host with
HIPIE_EINVAL and a message that starts with the entry's name and reports BH and N; nothing reaches a launch (the pointers are fake), so
no device is needed."""
import ctypes

import pytest

from hipie_amd import _lib

ENTRIES = (("hipie_attn_train_forward", b"attn_train_forward: ", 8), ("hipie_attn_train_backward", b"attn_train_backward: ", 13))


def _call(lib, name, n_ptr, BH=2, N=256, null=None):
    a = [ctypes.c_void_p(4096 * (k + 1)) for k in range(n_ptr)]
    if null is not None:
        a[null] = None
    return getattr(lib, name)(*a, BH, N, None)


@pytest.mark.parametrize("name,prefix,n_ptr", ENTRIES)
@pytest.mark.parametrize("kw", [dict(N=0), dict(N=127), dict(N=129), dict(N=-5), dict(BH=0), dict(BH=-1)], ids=lambda kw: "%s=%d" % next(iter(kw.items())))
def test_shape_refused_on_the_host(name, prefix, n_ptr, kw):
    lib = _lib.load()
    assert len(_lib.SIGNATURES[name]) == n_ptr + 3
    assert _call(lib, name, n_ptr, **kw) == -22
    err = lib.hipie_last_error()
    assert err == prefix + b"BH=%d N=%d (N a multiple of 128)" % (kw.get("BH", 2), kw.get("N", 256)), err


@pytest.mark.parametrize("name,prefix,n_ptr", ENTRIES)
def test_each_null_pointer_refused_on_the_host(name, prefix, n_ptr):
    lib = _lib.load()
    for i in range(n_ptr):
        assert _call(lib, name, n_ptr, null=i) == -22, i
        assert lib.hipie_last_error() == prefix + b"null pointer", (i, lib.hipie_last_error())
        # the pointers are looked at before the shape
        assert _call(lib, name, n_ptr, N=127, null=i) == -22 and lib.hipie_last_error() == prefix + b"null pointer", i
