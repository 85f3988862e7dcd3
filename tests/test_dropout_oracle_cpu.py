"""CPU checks of the dropout oracle (tests/dropout_oracle.py) that the GPU
dropout tests rely on: its attention reference, the statistics of its mask,
and a control showing that the GPU tolerances can see a wrong mask."""

import math

import numpy as np
import pytest
import torch

from tests.dropout_oracle import (attn_keep_mask, drop_threshold_u8,
                                  elem_keep_mask, keep_rate, keep_scale,
                                  ref_attention_masked)

# the bounds of tests/gpu/test_dropout_exact_gpu.py
FWD_TOL = 2e-2    # max-abs, times 1 / (1 - p)
GRAD_TOL = 5e-2   # relative to the reference grad's max-abs

SEEDS = [0x1234567, 987654321012345, (1 << 61) + 0xDEADBEEF]


def _bf16_randn(*shape):
    return torch.randn(*shape).to(torch.bfloat16).float()


# 1. reference check -------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hkv", [4, 2])
def test_ref_attention_all_ones_mask_is_plain_attention(causal, hkv):
    torch.manual_seed(0)
    b, s, h, d = 2, 40, 4, 16
    q, k, v = _bf16_randn(b, s, h, d), _bf16_randn(b, s, hkv, d), _bf16_randn(b, s, hkv, d)
    scale = 1.0 / math.sqrt(d)
    ones = torch.ones(b * h, s, s, dtype=torch.bool)
    got = ref_attention_masked(q, k, v, scale, ones, 1.0, causal)

    g = h // hkv
    sc = torch.einsum("bihd,bjhd->bhij", q, k.repeat_interleave(g, dim=2)) * scale
    if causal:
        sc = sc.masked_fill(~torch.ones(s, s, dtype=torch.bool).tril_(), float("-inf"))
    want = torch.einsum("bhij,bjhd->bihd", torch.softmax(sc, -1),
                        v.repeat_interleave(g, dim=2))
    assert (got - want).abs().max().item() < 1e-5


def test_ref_attention_masking_conventions():
    """kv_len, window and ALiBi follow the kernels' conventions; a row without
    a visible key gives zeros."""
    torch.manual_seed(1)
    b, s, h, d = 2, 24, 2, 8
    q, k, v = _bf16_randn(b, s, h, d), _bf16_randn(b, s, h, d), _bf16_randn(b, s, h, d)
    ones = torch.ones(b * h, s, s, dtype=torch.bool)
    lens = torch.tensor([s, 5])
    o = ref_attention_masked(q, k, v, 0.3, ones, 1.0, True, kv_len=lens, window=4)
    # batch 1: queries i >= 5 + 3 see no key (j < 5 and i - j < 4)
    assert o[1, 8:].abs().max().item() == 0.0
    assert o[1, :8].abs().min().item() > 0.0
    # window 1: each query sees only itself
    o1 = ref_attention_masked(q, k, v, 0.3, ones, 1.0, True, window=1)
    assert (o1 - v).abs().max().item() < 1e-6
    # a huge negative slope on (j - i) <= 0 leaves only the diagonal as well
    slopes = torch.full((h,), 1.0e4)
    oa = ref_attention_masked(q, k, v, 0.3, ones, 1.0, True, alibi_slopes=slopes)
    assert (oa - v).abs().max().item() < 1e-6


def test_thresholds_and_scales():
    assert drop_threshold_u8(0.1) == 26 and drop_threshold_u8(0.5) == 128
    assert drop_threshold_u8(0.3) == 77 and drop_threshold_u8(0.0) == 0
    assert drop_threshold_u8(0.999) == 255
    assert keep_rate(0.1) == 230 / 256
    assert keep_scale(0.5) == np.float32(2.0)
    assert keep_scale(0.1) == np.float32(1.0) / np.float32(0.9)
    assert attn_keep_mask(3, 2, 5, 8, 0.0).all()


def test_elem_mask_is_the_attention_hash_on_a_flat_index():
    """rnd_hash(seed, idx) is rnd_hash2(seed, idx & 0xffffffff, idx >> 32): for
    one head and one query row the two masks are the same bytes."""
    for seed in SEEDS:
        a = attn_keep_mask(seed, 1, 1, 1024, 0.3)[0, 0]
        e = elem_keep_mask(seed, 1024, 0.3)
        assert torch.equal(a, e)
        assert elem_keep_mask(seed, 1021, 0.3).shape == (1021,)
        assert torch.equal(elem_keep_mask(seed, 1021, 0.3), e[:1021])


# 2. statistics -------------------------------------------------------------------
def _ncorr(a, b, k):
    """Normalised correlation of two keep masks with keep rate k."""
    a = a.double() - k
    b = b.double() - k
    return (a * b).mean().item() / (k * (1.0 - k)), a.numel()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_attn_keep_mask_statistics(p, seed):
    BH, S = 8, 384
    m = attn_keep_mask(seed, BH, S, S, p)
    assert m.shape == (BH, S, S) and m.dtype == torch.bool
    k = keep_rate(p)

    def sigma(n):
        return math.sqrt(k * (1.0 - k) / n)

    worst = 0.0
    for bh in range(BH):
        z = abs(m[bh].double().mean().item() - k) / sigma(S * S)
        worst = max(worst, z)
        assert z < 5.0, f"head {bh}: keep rate off by {z:.2f} sigma"
    for lane in range(4):
        sub = m[:, :, lane::4]
        z = abs(sub.double().mean().item() - k) / sigma(sub.numel())
        worst = max(worst, z)
        assert z < 5.0, f"byte lane {lane}: keep rate off by {z:.2f} sigma"

    m1 = attn_keep_mask(seed + 1, BH, S, S, p)
    pairs = {
        "adjacent heads": (m[:-1], m[1:]),
        "adjacent queries": (m[:, :-1], m[:, 1:]),
        "adjacent keys": (m[:, :, :-1], m[:, :, 1:]),
        "seed vs seed+1": (m, m1),
    }
    for name, (a, b) in pairs.items():
        c, n = _ncorr(a, b, k)
        z = abs(c) * math.sqrt(n)  # sigma of the normalised correlation: 1/sqrt(n)
        worst = max(worst, z)
        assert z < 5.0, f"{name}: correlation {c:.3e} is {z:.2f} sigma"
    print(f"p={p} seed={seed:#x}: worst deviation {worst:.2f} sigma")


# 3. sensitivity control -------------------------------------------------------------
@pytest.mark.parametrize("hkv", [4, 1])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("s,d", [(200, 64), (384, 128)])
def test_tolerances_can_see_a_wrong_mask(s, d, p, causal, hkv):
    """A mask shifted by one key, one head or one query moves the forward
    output and every gradient by at least 4x the GPU tests' tolerances."""
    torch.manual_seed(0)
    b, h = 2, 4
    q, k, v = _bf16_randn(b, s, h, d), _bf16_randn(b, s, hkv, d), _bf16_randn(b, s, hkv, d)
    g = _bf16_randn(b, s, h, d)
    scale = 1.0 / math.sqrt(d)
    keep = attn_keep_mask(SEEDS[2], b * h, s, s, p)
    ks = float(keep_scale(p))

    def run(mask):
        qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
        o = ref_attention_masked(qr, kr, vr, scale, mask, ks, causal)
        o.backward(g)
        return o.detach(), qr.grad, kr.grad, vr.grad

    base = run(keep)
    for name, dim in (("key", 2), ("head", 0), ("query", 1)):
        other = run(torch.roll(keep, 1, dims=dim))
        fwd = (base[0] - other[0]).abs().max().item()
        assert fwd >= 4 * FWD_TOL / (1 - p), f"{name}-rolled mask: fwd diff {fwd}"
        for gname, a, c in zip(("dq", "dk", "dv"), base[1:], other[1:]):
            rel = ((a - c).abs().max() / a.abs().max()).item()
            assert rel >= 4 * GRAD_TOL, f"{name}-rolled mask: {gname} rel diff {rel}"
