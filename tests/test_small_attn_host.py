"""What ops.attn_f32, ops.attn_split and ops.attn_f32_rows refuse on the host before anything reaches the library: the kernels index k, v
and the mask by q's B, H, hd and k's Nk (hipie_amd/csrc/attn_f32.hip, attn_split.hip), so operands that disagree about them would be
read out of bounds.  Runs on the CPU: ops._on_device is a no-op here and ops._call fails the test when it is reached, so no mismatched
launch is ever made.  The conformance of the kernels themselves is tests/test_gpu_small_attn.py."""
import pytest
import torch

from hipie_amd import ops

B, H, HD, NQ, NK = 2, 3, 32, 5, 7


def f32(*s):
    return torch.zeros(*s)


def u8(*s):
    return torch.ones(*s, dtype=torch.uint8)


@pytest.fixture
def reached(monkeypatch):
    """the ops on host tensors with the library stubbed out: -> the list of entry points a test reached"""
    calls = []
    monkeypatch.setattr(ops, "_on_device", lambda op, names, *tensors: None)
    monkeypatch.setattr(ops, "_call", lambda name, *a: calls.append(name))
    return calls


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(ops, "_on_device", lambda op, names, *tensors: None)
    monkeypatch.setattr(ops, "_call", lambda name, *a: pytest.fail("%s reached the library" % name))


OPS = {
    "attn_f32": lambda q, k, v, m: ops.attn_f32(q, k, v, 1.0, key_mask=m),
    "attn_split": lambda q, k, v, m: ops.attn_split(q, k, v, 1.0, key_mask=m),
    "attn_f32_rows": lambda q, k, v, m: ops.attn_f32_rows(q, k, v, 1.0, m),
    "attn_split_rows": lambda q, k, v, m: ops.attn_f32_rows(q, k, v, 1.0, m, split=True),
}


def good(name):
    return [f32(B, NQ, H, HD), f32(B, NK, H, HD), f32(B, NK, H, HD), u8(B, NQ, NK) if name.endswith("rows") else u8(B, NK)]


# operand index, its replacement, what the message names
BAD = {
    "k-batch": (1, f32(B + 1, NK, H, HD), "k must be"), "k-heads": (1, f32(B, NK, H + 1, HD), "k must be"),
    "k-head-dim": (1, f32(B, NK, H, 64), "k must be"), "k-rank": (1, f32(B, NK, H * HD), "k must have 4 dimensions"),
    "v-batch": (2, f32(B - 1, NK, H, HD), "v must be"), "v-heads": (2, f32(B, NK, 1, HD), "v must be"),
    "v-head-dim": (2, f32(B, NK, H, 64), "v must be"), "v-keys": (2, f32(B, NK + 1, H, HD), "v must be"),
    "v-fewer-keys": (2, f32(B, NK - 1, H, HD), "v must be"), "q-rank": (0, f32(B, NQ, H * HD), "q must have 4 dimensions"),
}
BAD_KEY_MASK = {"mask-keys": u8(B, NK + 1), "mask-batch": u8(1, NK), "mask-rank": u8(B, 1, NK), "mask-rows": u8(B, NQ, NK), "mask-flat": u8(B * NK)}
BAD_ROW_MASK = {"mask-keys": u8(B, NQ, NK - 1), "mask-rows": u8(B, NQ + 1, NK), "mask-batch": u8(1, NQ, NK), "mask-key-mask": u8(B, NK),
                "mask-swapped": u8(B, NK, NQ)}


@pytest.mark.parametrize("name", sorted(OPS))
def test_agreeing_operands_reach_the_library(reached, name):
    out = OPS[name](*good(name))
    assert reached == ["hipie_" + name] and out.shape == (B, NQ, H * HD)


def test_no_mask_reaches_the_library(reached):
    for name in ("attn_f32", "attn_split"):
        OPS[name](*good(name)[:3], None)
    assert reached == ["hipie_attn_f32", "hipie_attn_split"]


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("name", sorted(OPS))
def test_disagreeing_operands_are_refused_before_the_library(no_library, name, bad):
    args = good(name)
    i, t, what = BAD[bad]
    args[i] = t
    with pytest.raises(RuntimeError, match=what):
        OPS[name](*args)


@pytest.mark.parametrize("name,bad", [(n, b) for n in sorted(OPS) for b in sorted(BAD_ROW_MASK if n.endswith("rows") else BAD_KEY_MASK)])
def test_a_mask_of_another_shape_is_refused_before_the_library(no_library, name, bad):
    args = good(name)
    args[3] = (BAD_ROW_MASK if name.endswith("rows") else BAD_KEY_MASK)[bad]
    with pytest.raises(RuntimeError, match="query_mask must be" if name.endswith("rows") else "key_mask must be"):
        OPS[name](*args)


def test_the_refusal_names_the_shapes(no_library):
    with pytest.raises(RuntimeError, match=r"hipie_attn_split: key_mask must be \(2, 7\), got \(2, 8\)"):
        ops.attn_split(*good("attn_split")[:3], 1.0, key_mask=u8(B, NK + 1))
    with pytest.raises(RuntimeError, match=r"attn_f32_rows: v must be \(2, 7, 3, 32\), got \(2, 8, 3, 32\)"):
        ops.attn_f32_rows(f32(B, NQ, H, HD), f32(B, NK, H, HD), f32(B, NK + 1, H, HD), 1.0, u8(B, NQ, NK))
