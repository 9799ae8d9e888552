"""Host-side refusals of the row kernels' entry points: hipie_add_layernorm / _rows / _sum / _dec, hipie_add_cast, hipie_layernorm_backward,
hipie_act_forward / _backward and hipie_group_norm (csrc/layernorm.hip, layernorm_bwd.hip, act_bwd.hip, groupnorm.hip).  Every call violates
ONE condition of the entry check, so it is refused on the host with HIPIE_EINVAL and the whole message is matched; the empty calls return 0
before anything is looked at that a launch would need.  Nothing reaches a launch (the pointers are fake), so no device is needed.

Left to tests/test_layernorm_bwd_cpu.py and tests/test_act_bwd_cpu.py, which pin them by a word of the message: the null-pointer, `go
together`, C / N, activation-code, workspace and alias refusals of hipie_layernorm_backward and hipie_act_forward / _backward, their empty
calls, and the monotonicity and saturation of the two workspace queries.  Here: their alignment refusal pointer by pointer, negative
rows, and the workspace sizes at the workgroup cap."""
import ctypes

import pytest

from hipie_amd import _lib

F32, F16, BF16, F64, HL8 = 0, 1, 2, 3, 4
P = [ctypes.c_void_p(4096 * (k + 1)) for k in range(8)]            # distinct, 4096-byte aligned
ODD = ctypes.c_void_p(4096 * 9 + 16)                                  # 16-byte but not 32-byte aligned
ODD4 = ctypes.c_void_p(4096 * 9 + 4)                                  # not 16-byte aligned


def _refused(name, args, message):
    lib = _lib.load()
    assert len(args) == len(_lib.SIGNATURES[name])
    assert getattr(lib, name)(*args) == -22, (name, args)
    assert lib.hipie_last_error() == message, lib.hipie_last_error()


def _accepted(name, args):
    assert getattr(_lib.load(), name)(*args) == 0, (name, _lib.load().hipie_last_error())


# ------------------------------------------------------------------------------------------------ hipie_add_layernorm, _rows, _sum
def _ln(entry, x=P[0], delta=P[1], gamma=P[2], beta=P[3], res=P[4], norm=P[5], rows=8, C=256, xd=F32, dd=F32, nd=F32, extra=None):
    head = [x, delta, gamma, beta, res, norm]
    tail = [rows, C, 1e-5, xd, dd, nd]
    if entry == "hipie_add_layernorm":
        return head + tail + [None]
    if entry == "hipie_add_layernorm_rows":
        return head + tail + list(extra or (P[6], P[7])) + [None]
    return head + list(extra or (P[6], P[7])) + tail + [None]          # _sum: addend, sum_out


LN_ENTRIES = ("hipie_add_layernorm", "hipie_add_layernorm_rows", "hipie_add_layernorm_sum")
LN_C = b"add_layernorm: C=%d must be a multiple of 4 and <= 2048"
LN_CASES = [(dict(**{n: None}), b"add_layernorm: null pointer") for n in ("x", "gamma", "beta", "norm")]
LN_CASES += [(dict(C=C), LN_C % C) for C in (0, -4, 6, 254, 2052, 4096)]
LN_CASES += [(dict(rows=-1), LN_C % 256)]
LN_CASES += [(dict(xd=d), b"add_layernorm: bad x dtype %d" % d) for d in (F64, HL8, 5, -1)]
LN_CASES += [(dict(dd=d), b"add_layernorm: bad delta dtype %d" % d) for d in (F64, HL8, 5, -1)]
LN_CASES += [(dict(nd=d), b"add_layernorm: bad norm dtype %d" % d) for d in (F64, 5, -1)]
LN_CASES += [(dict(nd=HL8, **kw), b"add_layernorm: HL8 output needs C % 8 == 0 and a 32-byte aligned buffer") for kw in (dict(C=12), dict(C=260), dict(norm=ODD))]
# the order of the checks: pointers, C, then the dtypes x, delta, norm
LN_CASES += [(dict(x=None, C=6, xd=9), b"add_layernorm: null pointer"), (dict(C=6, xd=9), LN_C % 6),
             (dict(xd=9, dd=9, nd=9), b"add_layernorm: bad x dtype 9"), (dict(dd=9, nd=9), b"add_layernorm: bad delta dtype 9"),
             (dict(dd=9, nd=HL8, C=12), b"add_layernorm: bad delta dtype 9")]


@pytest.mark.parametrize("entry", LN_ENTRIES)
@pytest.mark.parametrize("kw,message", LN_CASES, ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_add_layernorm_refusals(entry, kw, message):
    _refused(entry, _ln(entry, **kw), message)


@pytest.mark.parametrize("entry", LN_ENTRIES)
def test_add_layernorm_without_rows_returns_before_the_dtypes(entry):
    _accepted(entry, _ln(entry, rows=0))
    _accepted(entry, _ln(entry, rows=0, delta=None, res=None, xd=9, dd=9, nd=9))
    _refused(entry, _ln(entry, rows=0, C=6), LN_C % 6)
    _refused(entry, _ln(entry, rows=0, x=None), b"add_layernorm: null pointer")


def test_add_layernorm_sum_pairs_its_two_pointers():
    for extra in ((P[6], None), (None, P[7])):
        _refused("hipie_add_layernorm_sum", _ln("hipie_add_layernorm_sum", extra=extra), b"add_layernorm_sum: addend and sum_out go together")
        _refused("hipie_add_layernorm_sum", _ln("hipie_add_layernorm_sum", extra=extra, x=None, rows=0), b"add_layernorm_sum: addend and sum_out go together")


# ------------------------------------------------------------------------------------------------ hipie_add_layernorm_dec
def _dec(x=P[0], delta=P[1], gamma=P[2], beta=P[3], norm=P[4], norm16=P[5], addend=P[6], sum16=P[7], rows=8, C=256, dd=F32, ad=F16):
    return [x, delta, gamma, beta, norm, norm16, addend, sum16, rows, C, 1e-5, dd, ad, None]


DEC_C = b"add_layernorm_dec: C=%d must be a multiple of 4 and <= 2048"
DEC_CASES = [(dict(**{n: None}), b"add_layernorm_dec: null pointer") for n in ("x", "delta", "gamma", "beta", "norm")]
DEC_CASES += [(dict(addend=None), b"add_layernorm_dec: sum16_out needs addend")]
DEC_CASES += [(dict(C=C), DEC_C % C) for C in (0, -4, 6, 254, 2052)] + [(dict(rows=-1), DEC_C % 256)]
DEC_CASES += [(dict(ad=d), b"add_layernorm_dec: aux dtype must be f16, bf16 or HL8") for d in (F32, F64, 5, -1)]
DEC_CASES += [(dict(ad=HL8, **kw), b"add_layernorm_dec: HL8 outputs need C % 8 == 0 and 32-byte aligned buffers")
              for kw in (dict(C=12), dict(norm16=ODD), dict(addend=ODD), dict(sum16=ODD))]
DEC_CASES += [(dict(dd=d, ad=ad), b"add_layernorm_dec: bad delta dtype %d" % d) for d in (F64, HL8, 5, -1) for ad in (F16, BF16, HL8)]
DEC_CASES += [(dict(x=None, addend=None, C=6), b"add_layernorm_dec: null pointer"), (dict(addend=None, C=6), b"add_layernorm_dec: sum16_out needs addend"),
              (dict(C=6, ad=F32, dd=9), DEC_C % 6), (dict(ad=F32, dd=9), b"add_layernorm_dec: aux dtype must be f16, bf16 or HL8")]


@pytest.mark.parametrize("kw,message", DEC_CASES, ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_add_layernorm_dec_refusals(kw, message):
    _refused("hipie_add_layernorm_dec", _dec(**kw), message)


def test_add_layernorm_dec_without_rows():
    _accepted("hipie_add_layernorm_dec", _dec(rows=0))
    _accepted("hipie_add_layernorm_dec", _dec(rows=0, norm16=None, addend=None, sum16=None, dd=9, ad=HL8))
    _refused("hipie_add_layernorm_dec", _dec(rows=0, ad=F32), b"add_layernorm_dec: aux dtype must be f16, bf16 or HL8")


# ------------------------------------------------------------------------------------------------ hipie_add_cast
def _cast(a=P[0], b=P[1], out=P[2], n=1024, dtype=F16):
    return [a, b, out, n, dtype, None]


CAST_CASES = [(dict(**{n: None}), b"add_cast: null pointer") for n in ("a", "b", "out")]
CAST_CASES += [(dict(n=n), b"add_cast: n must be a multiple of 4") for n in (-4, -1, 6, 1023)]
CAST_CASES += [(dict(dtype=d), b"add_cast: dtype must be f16, bf16 or HL8") for d in (F32, F64, 5, -1)]
CAST_CASES += [(dict(dtype=HL8, **kw), b"add_cast: HL8 needs n % 8 == 0 and 32-byte aligned buffers") for kw in (dict(n=12), dict(b=ODD), dict(out=ODD))]
CAST_CASES += [(dict(a=None, n=6, dtype=F32), b"add_cast: null pointer"), (dict(n=6, dtype=F32), b"add_cast: n must be a multiple of 4")]


@pytest.mark.parametrize("kw,message", CAST_CASES, ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_add_cast_refusals(kw, message):
    _refused("hipie_add_cast", _cast(**kw), message)


def test_add_cast_of_nothing():
    for d in (F16, BF16, HL8):
        _accepted("hipie_add_cast", _cast(n=0, dtype=d))
    _refused("hipie_add_cast", _cast(n=0, dtype=F32), b"add_cast: dtype must be f16, bf16 or HL8")


# ------------------------------------------------------------------------------------------------ hipie_layernorm_backward
def _lnb(s=P[0], gy=P[1], gres=P[2], gamma=P[3], dx=P[4], dgamma=P[5], dbeta=P[6], ws=P[7], ws_bytes=1 << 40, rows=8, C=256):
    return [s, gy, gres, gamma, dx, dgamma, dbeta, ws, ws_bytes, rows, C, 1e-5, None]


@pytest.mark.parametrize("name", ["s", "gy", "gres", "gamma", "dx", "ws"])
def test_layernorm_backward_alignment(name):
    _refused("hipie_layernorm_backward", _lnb(**{name: ODD4}), b"layernorm_backward: buffers must be 16-byte aligned")


def test_layernorm_backward_messages_and_order():
    C = b"layernorm_backward: C=%d must be a multiple of 4 and <= 2048"
    _refused("hipie_layernorm_backward", _lnb(rows=-1), C % 256)
    _refused("hipie_layernorm_backward", _lnb(C=6, dgamma=None, s=None), C % 6)
    _refused("hipie_layernorm_backward", _lnb(dgamma=None, s=None), b"layernorm_backward: dgamma and dbeta go together (both or neither)")
    _refused("hipie_layernorm_backward", _lnb(s=None, dx=P[1]), b"layernorm_backward: null pointer")
    _refused("hipie_layernorm_backward", _lnb(dx=P[1], gy=P[1], ws=ODD4), b"layernorm_backward: dx must not alias s or gy (only gres)")
    need = _lib.load().hipie_layernorm_backward_ws_bytes(8, 256)
    _refused("hipie_layernorm_backward", _lnb(ws_bytes=need - 1), b"layernorm_backward: workspace of %d bytes, need %d" % (need - 1, need))
    # without rows and without parameter gradients nothing is looked at but C and the pairing
    _accepted("hipie_layernorm_backward", _lnb(rows=0, s=None, gy=None, gamma=None, dx=None, dgamma=None, dbeta=None, ws=None, ws_bytes=0))
    _refused("hipie_layernorm_backward", _lnb(rows=0, C=2052, dgamma=None, dbeta=None), C % 2052)


def test_layernorm_backward_workspace_at_the_workgroup_cap():
    """one partial row of 2 C floats per workgroup of 4 rows, at most 1024 workgroups"""
    ws = _lib.load().hipie_layernorm_backward_ws_bytes
    for C in (4, 256, 2048):
        row = 2 * C * 4
        assert ws(0, C) == 16 and ws(-3, C) == 16 and ws(8, 0) == 16
        assert [ws(r, C) for r in (1, 4, 5)] == [row, row, 2 * row]
        assert [ws(r, C) for r in (4092, 4093, 4096, 4097, 4100, 1 << 40)] == [1023 * row] + [1024 * row] * 5


# ------------------------------------------------------------------------------------------------ hipie_act_forward / _backward
def _actf(u=P[0], a=P[1], rows=8, N=256, act=1):
    return [u, a, rows, N, act, None]


def _actb(u=P[0], g=P[1], du=P[2], a=P[3], dbias=P[4], ws=P[5], rows=8, N=256, act=1):
    return [u, g, du, a, dbias, ws, rows, N, act, None]


@pytest.mark.parametrize("name", ["u", "a"])
def test_act_forward_alignment(name):
    _refused("hipie_act_forward", _actf(**{name: ODD4}), b"act_forward: buffers must be 16-byte aligned")


@pytest.mark.parametrize("name", ["u", "g", "du", "a", "dbias", "ws"])
def test_act_backward_alignment(name):
    _refused("hipie_act_backward", _actb(**{name: ODD4}), b"act_backward: buffers must be 16-byte aligned")


def test_act_messages_and_order():
    _refused("hipie_act_forward", _actf(rows=-1), b"act_forward: rows=-1, N=256: N must be a multiple of 4")
    _refused("hipie_act_forward", _actf(N=6, act=3, u=None), b"act_forward: rows=8, N=6: N must be a multiple of 4")
    _refused("hipie_act_forward", _actf(act=3, u=None), b"act_forward: act=3 must be 1 (GELU) or 2 (ReLU)")
    _refused("hipie_act_forward", _actf(u=None, a=ODD4), b"act_forward: null pointer")
    _refused("hipie_act_forward", _actf(a=P[0]), b"act_forward: a must not alias u")
    _refused("hipie_act_backward", _actb(rows=-1), b"act_backward: rows=-1, N=256: N must be a multiple of 4")
    _refused("hipie_act_backward", _actb(N=6, act=3, ws=None), b"act_backward: rows=8, N=6: N must be a multiple of 4")
    _refused("hipie_act_backward", _actb(act=3, ws=None), b"act_backward: act=3 must be 1 (GELU) or 2 (ReLU)")
    _refused("hipie_act_backward", _actb(ws=None, u=None), b"act_backward: dbias needs the workspace of hipie_act_backward_ws_bytes")
    _refused("hipie_act_backward", _actb(u=None, du=ODD4), b"act_backward: null pointer")
    _refused("hipie_act_backward", _actb(du=P[0], ws=ODD4), b"act_backward: du must not alias u, a must not alias u, g or du (du may alias g)")
    # du may be g; without dbias nothing is zero-filled for empty work
    _refused("hipie_act_backward", _actb(du=P[1], a=P[1]), b"act_backward: du must not alias u, a must not alias u, g or du (du may alias g)")
    _accepted("hipie_act_backward", _actb(rows=0, u=None, g=None, du=None, a=None, dbias=None, ws=None))
    _accepted("hipie_act_backward", _actb(N=0, u=None, g=None, du=None, a=None, dbias=None, ws=None))


def test_act_backward_workspace_at_the_workgroup_cap():
    """one partial row of N floats per chunk of 4 rows, at most max(1, 2048 / ceil(N / 1024)) chunks"""
    ws = _lib.load().hipie_act_backward_ws_bytes
    assert [ws(r, 1 << 22) for r in (1, 5, 1 << 40)] == [4 << 22] * 3            # more column tiles than workgroups: one chunk
    for N, cap in ((4, 2048), (256, 2048), (1024, 2048), (1028, 1024), (5120, 409), (1 << 20, 2)):
        row = N * 4
        assert ws(0, N) == 16 and ws(-3, N) == 16 and ws(8, 0) == 16
        assert [ws(r, N) for r in (1, 4, 5)] == [row, row, min(2, cap) * row]
        assert [ws(r, N) for r in (4 * cap - 4, 4 * cap - 3, 4 * cap, 4 * cap + 1, 4 * cap + 4, 1 << 40)] == [max(cap - 1, 1) * row] + [cap * row] * 5


# ------------------------------------------------------------------------------------------------ hipie_group_norm
def _gn(x=P[0], prebias=P[1], gamma=P[2], beta=P[3], out=P[4], ws=P[5], B=2, C=256, HW=64, groups=32, cl=0, relu=0, xd=F32, od=F32):
    return [x, prebias, gamma, beta, out, ws, B, C, HW, groups, cl, 1e-5, relu, xd, od, None]


GN_GROUPS = b"group_norm: %d channels in %d groups unsupported (8 channels per group, 256 %% groups == 0)"
GN_CL = b"group_norm: channels_last %d (0 NCHW, 1 channels-last, 2 channels-last in / NCHW out: H*W %% 64 == 0, got %d)"
GN_CASES = [(dict(**{n: None}), b"group_norm: null pointer") for n in ("x", "gamma", "beta", "out", "ws")]
GN_CASES += [(kw, b"group_norm: bad shape") for kw in (dict(B=-1), dict(C=0, groups=0), dict(C=-8, groups=-1), dict(HW=0), dict(HW=-64))]
GN_CASES += [(dict(C=C, groups=g), GN_GROUPS % (C, g)) for C, g in ((256, 0), (256, -32), (256, 16), (260, 32), (1024, 128), (24, 3), (96, 12))]
GN_CASES += [(dict(HW=HW), b"group_norm: NCHW needs H*W %% 8 == 0 (got %d)" % HW) for HW in (1, 63, 68)]
GN_CASES += [(dict(cl=cl, HW=HW), GN_CL % (cl, HW)) for cl, HW in ((3, 64), (-1, 64), (2, 63), (2, 96), (2, 8))]
GN_CASES += [(dict(xd=d, cl=cl), b"group_norm: bad x dtype %d" % d) for d in (F64, HL8, 5, -1) for cl in (0, 1, 2)]
GN_CASES += [(dict(od=d, cl=cl), b"group_norm: bad out dtype %d" % d) for d in (F64, HL8, 5, -1) for cl in (0, 1, 2)]
GN_CASES += [(dict(x=None, B=-1), b"group_norm: null pointer"), (dict(B=-1, groups=3), b"group_norm: bad shape"),
             (dict(groups=3, HW=63), GN_GROUPS % (256, 3)), (dict(HW=63, cl=3), GN_CL % (3, 63)), (dict(cl=3, xd=9), GN_CL % (3, 64)),
             (dict(xd=9, od=9), b"group_norm: bad x dtype 9")]


@pytest.mark.parametrize("kw,message", GN_CASES, ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_group_norm_refusals(kw, message):
    _refused("hipie_group_norm", _gn(**kw), message)


def test_group_norm_of_no_image():
    _accepted("hipie_group_norm", _gn(B=0))
    _accepted("hipie_group_norm", _gn(B=0, prebias=None, cl=1, HW=63, xd=9, od=9))
    _refused("hipie_group_norm", _gn(B=0, HW=63), b"group_norm: NCHW needs H*W % 8 == 0 (got 63)")
