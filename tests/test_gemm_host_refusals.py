"""Host-side refusals of the split-GEMM family: hipie_gemm, _gather, _batched, _batched_resid, _batched_softmax, _batched_softmax_bias,
hipie_gemm_ln, hipie_gemm_f8x and hipie_conv3x3_split.

Every call below violates exactly ONE condition of its entry point (and none that is checked before it), so it is refused on the host:
rc == HIPIE_EINVAL, and hipie_last_error() starts with the entry point's prefix and names the check (and the values it reports).  Nothing
reaches a launch: the pointers are fake (256: 16-byte aligned, 264: not) and no device is needed.  `GOOD[name]` is an argument set that
passes every check of `name`; it is never called as it stands.
"""
import ctypes

import pytest

from hipie_amd import _lib

F32, F16, HL8 = 0, 1, 4
P = ctypes.c_void_p(256)          # 16-byte aligned
ODD = ctypes.c_void_p(264)        # 8 bytes past a 16-byte boundary
BIG = 1 << 22                     # row stride in fp16 elements: 256 rows x 2^22 x 2 bytes = 2^31
LDW_256_ONLY = 3355448            # % 8 == 0; 256 * ldw * 2 < 2^31 <= 320 * ldw * 2: fits the 256-column tile's limit only

ORDER = {
    "hipie_gemm": "A lda W ldw bias resid ldr out ldo out_row M N K in_fmt out_fmt act alpha oscale stream",
    "hipie_gemm_gather": "A lda a_rows a_row W ldw bias resid ldr out ldo out_row M N K in_fmt out_fmt act alpha oscale stream",
    "hipie_gemm_batched": "A lda a_outer a_inner W ldw w_outer w_inner out ldo o_outer o_inner n_outer n_inner M N K out_fmt alpha stream",
    "hipie_gemm_batched_resid": "A lda a_outer a_inner W ldw w_outer w_inner bias resid ldr r_outer r_inner out ldo o_outer o_inner "
                                "n_outer n_inner M N K alpha stream",
    "hipie_gemm_batched_softmax": "A lda a_outer a_inner W ldw w_outer w_inner out ldo o_outer o_inner n_outer n_inner M N K mask L clamp "
                                  "alpha stream",
    "hipie_gemm_batched_softmax_bias": "A lda a_outer a_inner W ldw w_outer w_inner out ldo o_outer o_inner n_outer n_inner M N K mask L "
                                       "col_bias clamp alpha stream",
    "hipie_gemm_ln": "A lda W ldw bias resid ldr gamma beta eps out ldo out_hl8 ldo_hl8 M K in_fmt alpha stream",
    "hipie_gemm_f8x": "A lda W ldw w_scale bias resid ldr out ldo out_row M N K in_fmt out_fmt act alpha oscale stream",
    "hipie_conv3x3_split": "x ldx w bias out ldo rows Wp C N in_fmt out_fmt act stream",
}

_plain = dict(A=P, lda=128, W=P, ldw=128, bias=P, resid=P, ldr=64, out=P, ldo=64, out_row=None, M=10, N=64, K=64, in_fmt=HL8, out_fmt=F32,
              act=0, alpha=1.0, oscale=1.0, stream=None)
_batched = dict(A=P, lda=128, a_outer=1024, a_inner=128, W=P, ldw=128, w_outer=1024, w_inner=128, out=P, ldo=128, o_outer=2048,
                o_inner=128, n_outer=2, n_inner=2, M=10, N=64, K=64, alpha=1.0, stream=None)
GOOD = {
    "hipie_gemm": _plain,
    "hipie_gemm_gather": dict(_plain, a_rows=16, a_row=P),
    "hipie_gemm_batched": dict(_batched, out_fmt=F32),
    "hipie_gemm_batched_resid": dict(_batched, bias=P, resid=P, ldr=64, r_outer=1024, r_inner=64),
    "hipie_gemm_batched_softmax": dict(_batched, mask=P, L=60, clamp=0.0),
    "hipie_gemm_batched_softmax_bias": dict(_batched, mask=P, L=60, col_bias=P, clamp=0.0),
    "hipie_gemm_ln": dict(A=P, lda=128, W=P, ldw=128, bias=P, resid=P, ldr=256, gamma=P, beta=P, eps=1e-5, out=P, ldo=256, out_hl8=P,
                          ldo_hl8=512, M=10, K=64, in_fmt=HL8, alpha=1.0, stream=None),
    "hipie_gemm_f8x": dict(_plain, w_scale=P),
    "hipie_conv3x3_split": dict(x=P, ldx=128, w=P, bias=P, out=P, ldo=64, rows=100, Wp=10, C=64, N=64, in_fmt=HL8, out_fmt=F32, act=0,
                                stream=None),
}

# (entry point, message prefix, the arguments that differ from GOOD, what the message must contain)
CASES = []


def _add(name, prefix, *rows):
    CASES.extend((name, prefix, change, want if isinstance(want, tuple) else (want,)) for change, want in rows)


def _operand_checks():
    """what every entry point with two split operands checks: both row strides, and the 31-bit limit at a stride no tile width allows"""
    return [
        (dict(lda=120), b"operand row strides 120 / 128"),
        (dict(ldw=120), b"operand row strides 128 / 120"),
        (dict(lda=132), b"operand row strides 132 / 128"),
        (dict(ldw=132), b"operand row strides 128 / 132"),
        (dict(lda=BIG), b"row stride too large"),
        (dict(ldw=BIG), b"row stride too large"),
    ]


def _batch_checks():
    return [
        (dict(n_outer=0), b"0 x 2 problems"),
        (dict(n_inner=-1), b"2 x -1 problems"),
        (dict(n_outer=256, n_inner=256), b"256 x 256 problems"),          # 65536 > the 65535 blocks of gridDim.y
        (dict(a_outer=1028), b"batch offsets"),
        (dict(a_inner=4), b"batch offsets"),
        (dict(w_outer=1028), b"batch offsets"),
        (dict(w_inner=4), b"batch offsets"),
        (dict(o_outer=2050), b"batch offsets"),
        (dict(o_inner=2), b"batch offsets"),
    ]


def _misaligned(*names):
    return [({n: ODD}, b"16-byte aligned") for n in names]


for _name, _prefix in (("hipie_gemm", b"gemm: "), ("hipie_gemm_f8x", b"gemm_f8x: ")):
    _add(_name, _prefix,
         (dict(A=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(out=None), b"null pointer"),
         (dict(in_fmt=2), b"operand format 2"),
         (dict(out_fmt=2), b"output format 2"),
         (dict(act=4), b"activation 4"), (dict(act=-1), b"activation -1"),
         (dict(M=0), b"M=0 N=64 K=64"), (dict(N=12, ldo=12, ldr=12), b"M=10 N=12 K=64"), (dict(K=0), b"M=10 N=64 K=0"),
         (dict(K=48), b"K=48"),
         *_operand_checks(),
         (dict(ldw=LDW_256_ONLY), b"row stride too large"),           # the W tile is up to 320 rows
         (dict(ldo=60), b"output row stride 60 (>= 64)"),
         (dict(ldo=66), b"output row stride 66 (>= 64)"),
         (dict(out_fmt=HL8, ldo=64), b"output row stride 64 (>= 128)"),
         (dict(out_fmt=F16, ldo=60), b"output row stride 60 (>= 64)"),
         (dict(ldr=60), b"residual row stride 60"),
         (dict(ldr=66), b"residual row stride 66"),
         (dict(resid=None, ldr=0, out=ODD), b"16-byte aligned"),       # no residual: its stride is not looked at
         *_misaligned("A", "W", "out", "bias", "resid"))
_add("hipie_gemm", b"gemm: ",
     (dict(in_fmt=F16, K=96, lda=96, ldw=96), b"K=96 must be a multiple of 64"),     # plain fp16 operands: 64 elements per k tile
     (dict(in_fmt=F16, lda=64, ldw=64, ldo=60), b"output row stride 60 (>= 64)"),    # ... and K elements per row: these strides pass
     (dict(in_fmt=F16, lda=56, ldw=64), b"operand row strides 56 / 64"),
     (dict(in_fmt=F32, lda=60), b"operand row strides 120 / 128"),                   # fp32 A rows: lda in fp32 elements, reported in fp16 units
     (dict(in_fmt=F32, lda=BIG // 2), b"row stride too large"))
_add("hipie_gemm_f8x", b"gemm_f8x: ",
     (dict(w_scale=None), b"null pointer"),
     (dict(in_fmt=F32), b"operand format 0"), (dict(in_fmt=F16), b"operand format 1"))

_add("hipie_gemm_gather", b"gemm_gather: ",
     (dict(a_row=None), b"a_row map"), (dict(a_rows=0), b"a_row map"),
     (dict(in_fmt=F16), b"split operands only"),
     (dict(a_rows=1 << 24), b"below 4 GiB"),                          # 2^24 rows x 128 fp16 = 2^32 bytes
     (dict(in_fmt=F32, lda=64, a_rows=1 << 24), b"below 4 GiB"))      # 2^24 rows x 64 fp32
_add("hipie_gemm_gather", b"gemm: ",                                  # what it inherits from the plain GEMM keeps that prefix
     (dict(A=None), b"null pointer"), (dict(out_fmt=2), b"output format 2"), (dict(act=4), b"activation 4"), (dict(K=48), b"K=48"),
     (dict(N=12, ldo=12, ldr=12), b"N=12"),
     (dict(lda=120), b"operand row strides 120 / 128"), (dict(in_fmt=F32, lda=60), b"operand row strides 120 / 128"),
     (dict(ldw=LDW_256_ONLY), b"row stride too large"),
     (dict(ldo=60), b"output row stride 60 (>= 64)"), (dict(ldr=60), b"residual row stride 60"),
     *_misaligned("A", "W", "out", "bias", "resid"))

_add("hipie_gemm_batched", b"gemm_batched: ",
     (dict(A=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(out=None), b"null pointer"),
     (dict(out_fmt=F16), b"output format 1"),
     (dict(M=0), b"M=0 N=64 K=64"), (dict(N=12), b"M=10 N=12 K=64"), (dict(K=48), b"M=10 N=64 K=48"), (dict(K=0), b"K=0"),
     *_operand_checks(), *_batch_checks(),
     (dict(ldw=LDW_256_ONLY), b"row stride too large"),
     (dict(ldo=60), b"output row stride 60 (>= 64)"), (dict(ldo=66), b"output row stride 66 (>= 64)"),
     (dict(out_fmt=HL8, ldo=64), b"output row stride 64 (>= 128)"),
     *_misaligned("A", "W", "out"))

_add("hipie_gemm_batched_resid", b"gemm_batched_resid: ",
     (dict(A=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(out=None), b"null pointer"),
     (dict(M=0), b"M=0 N=64 K=64"), (dict(N=12), b"M=10 N=12 K=64"), (dict(K=48), b"M=10 N=64 K=48"),
     *_operand_checks(), *_batch_checks(),
     (dict(ldw=LDW_256_ONLY), b"row stride too large"),
     (dict(ldo=60), b"output row stride 60 (>= 64)"), (dict(ldo=66), b"output row stride 66 (>= 64)"),
     (dict(ldr=60), b"residual strides 60 / 1024 / 64"), (dict(ldr=66), b"residual strides 66 / 1024 / 64"),
     (dict(r_outer=1026), b"residual strides 64 / 1026 / 64"), (dict(r_inner=2), b"residual strides 64 / 1024 / 2"),
     (dict(resid=None, ldr=0, r_outer=2, out=ODD), b"16-byte aligned"),      # no residual: its strides are not looked at
     *_misaligned("A", "W", "out", "bias", "resid"))

for _name, _prefix in (("hipie_gemm_batched_softmax", b"gemm_batched_softmax: "), ("hipie_gemm_batched_softmax_bias", b"gemm_batched_softmax_bias: ")):
    _add(_name, _prefix,
         (dict(A=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(out=None), b"null pointer"),
         (dict(M=0), b"M=0 N=64 K=64 L=60"), (dict(N=12, L=10), b"M=10 N=12 K=64 L=10"), (dict(N=264, ldo=528), b"N=264"),
         (dict(K=48), b"K=48"), (dict(L=0), b"L=0"), (dict(L=65), b"L=65"),
         *_operand_checks(), *_batch_checks(),
         (dict(ldo=120), (b"output row stride 120", b">= 128)")), (dict(ldo=130), (b"output row stride 130", b">= 128)")),
         *_misaligned("A", "W", "out"))
_add("hipie_gemm_batched_softmax", b"gemm_batched_softmax: ", (dict(ldw=LDW_256_ONLY), b"row stride too large"))
_add("hipie_gemm_batched_softmax_bias", b"gemm_batched_softmax_bias: ",
     (dict(ldw=LDW_256_ONLY, ldo=120), b"output row stride 120"),     # one 256-column tile: this ldw is within the limit, the next check trips
     *_misaligned("col_bias"))

_add("hipie_gemm_ln", b"gemm_ln: ",
     *[({n: None}, b"null pointer") for n in ("A", "W", "out", "gamma", "beta", "resid")],
     (dict(in_fmt=F16), b"operand format 1"),
     (dict(M=0), b"M=0 K=64"), (dict(K=48), b"M=10 K=48"), (dict(K=0), b"K=0"),
     *_operand_checks(),
     (dict(in_fmt=F32, lda=60), b"operand row strides 120 / 128"),
     (dict(ldw=LDW_256_ONLY, ldo=200), b"output row stride 200 (>= 256)"),   # N = 256 = one 256-column tile: within the limit
     (dict(ldo=200), b"output row stride 200 (>= 256)"), (dict(ldo=258), b"output row stride 258 (>= 256)"),
     (dict(ldo_hl8=504), b"HL8 output row stride 504 (>= 512)"), (dict(ldo_hl8=516), b"HL8 output row stride 516 (>= 512)"),
     (dict(out_hl8=None, ldo_hl8=0, ldr=200), b"residual row stride 200"),   # no HL8 output: its stride is not looked at
     (dict(ldr=200), b"residual row stride 200"), (dict(ldr=258), b"residual row stride 258"),
     *_misaligned("A", "W", "out", "out_hl8", "bias", "resid"))

_add("hipie_conv3x3_split", b"conv3x3_split: ",
     (dict(x=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(out=None), b"null pointer"),
     (dict(in_fmt=F16), b"input format 1"),
     (dict(out_fmt=F16), b"output format 1"),
     (dict(act=3), b"activation 3"), (dict(act=-1), b"activation -1"),
     (dict(act=2, ldo=60), b"output row stride 60"),                  # ReLU is the last activation it takes: passes that check
     (dict(rows=0), b"rows=0 Wp=10 C=64 N=64"), (dict(rows=1 << 31), b"rows=2147483648"), (dict(Wp=2), b"Wp=2"), (dict(C=48), b"C=48"),
     (dict(C=0), b"C=0"), (dict(N=12), b"N=12"),
     (dict(ldx=120), b"input row stride 120"), (dict(ldx=132), b"input row stride 132"),
     (dict(in_fmt=F32, ldx=60), b"input row stride 120"),
     (dict(ldx=BIG), b"row stride too large"),
     (dict(ldx=(1 << 30) // 268 // 8 * 8 + 8), b"row stride too large"),     # (256 + Wp + 2) rows x ldx x 2 bytes just past 2^31
     (dict(ldx=(1 << 30) // 268 // 8 * 8, ldo=60), b"output row stride 60"),  # ... and just below it
     (dict(ldo=60), b"output row stride 60"), (dict(ldo=66), b"output row stride 66"),
     (dict(out_fmt=HL8, ldo=64), b"output row stride 64"),
     *_misaligned("x", "w", "out", "bias"))


def _id(case):
    name, prefix, change, _ = case
    return "%s-%s-%s" % (name[6:], prefix.decode().strip(": "), ",".join("%s=%s" % (k, getattr(v, "value", v)) for k, v in change.items()))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_every_entry_point_is_covered():
    assert {c[0] for c in CASES} == set(ORDER) and len(ORDER) == 9
    for name, args in GOOD.items():
        assert sorted(args) == sorted(ORDER[name].split()), name


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_refused_on_the_host(lib, case):
    name, prefix, change, wants = case
    args = dict(GOOD[name], **change)
    assert len(_lib.SIGNATURES[name]) == len(ORDER[name].split())
    rc = getattr(lib, name)(*[args[k] for k in ORDER[name].split()])
    err = lib.hipie_last_error()
    assert rc == -22, (rc, err)
    assert err.startswith(prefix), err
    for want in wants:
        assert want in err, (want, err)
