"""Flash-attention launch plumbing: every stride and pointer reaches the field
it belongs to.

q, k and v are views with nine pairwise different (batch, seq, head) strides
into three separately over-allocated buffers; the same call with
``.contiguous()`` copies must give the same bits, forward and backward, for
every kernel variant.  The arithmetic does not depend on addresses, so a
stride or pointer wired to the wrong argument is the only thing that can make
the two differ.  GQA (H = 4, Hkv = 2) gives dK/dV another shape than dQ and
exercises ``kv_group``; S = 160 is one full 128-row block plus a ragged one.
"""

import math

import pytest
import torch

from libai_amd.data.packing import doc_bounds_from_lengths
# the table gradient is summed with fp32 atomics (order dependent in its last
# bits): same error measure and bound as the rel-bias tests apply to it
from tests.gpu.test_flash_relbias_gpu import GRAD_TOL, _rel_err

pytestmark = pytest.mark.gpu

B, S, H, HKV = 2, 160, 4, 2
P_DROP = 0.1
SEED = (1 << 61) + 0xDEADBEEF  # the kernels fold seed >> 32 into the key
WINDOW = 40
# row 0 splits at 50, row 1 at 77: neither a multiple of 32
DOC_LENGTHS = ([50, 110], [77, 83])


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    from libai_amd.ops._ext import has_ext

    assert has_ext(), "HIP extension must be built+loaded on the GPU box"
    yield


def _ext():
    from libai_amd.ops._ext import ext

    return ext()


def _strided_view(gen, heads, d, pad_h, pad_s, pad_b, offset):
    """A [B, S, heads, d] bf16 view with padded head, seq and batch strides
    (elements; all multiples of 8, so every row stays 16-byte aligned) into a
    random buffer of its own."""
    sh = d + pad_h
    ss = heads * sh + pad_s
    sb = S * ss + pad_b
    buf = torch.randn(offset + B * sb, device="cuda", dtype=torch.float32,
                      generator=gen).to(torch.bfloat16)
    return buf.as_strided((B, S, heads, d), (sb, ss, sh, 1), offset)


def _views(d):
    gen = torch.Generator(device="cuda").manual_seed(d)
    q = _strided_view(gen, H, d, 8, 8, 16, 8)
    k = _strided_view(gen, HKV, d, 16, 24, 8, 16)
    v = _strided_view(gen, HKV, d, 24, 40, 24, 24)
    strides = [s for t in (q, k, v) for s in t.stride()[:3]]
    assert len(set(strides)) == 9, strides
    assert all(s % 8 == 0 for s in strides), strides
    assert q.stride(3) == k.stride(3) == v.stride(3) == 1
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    return q, k, v


def _variant_args(variant):
    """(alibi_slopes, window, rel_bias, doc_start, doc_end) of one variant."""
    gen = torch.Generator(device="cuda").manual_seed(17)
    slopes = table = ds = de = None
    window = 0
    if variant == "alibi":
        slopes = torch.tensor([2.0 ** -(i + 1) for i in range(H)], device="cuda",
                              dtype=torch.float32)
    elif variant == "window":
        window = WINDOW
    elif variant == "rel_bias":
        table = torch.randn(H, 2 * S - 1, device="cuda", dtype=torch.float32,
                            generator=gen) * 0.5
    elif variant == "docs":
        rows = [doc_bounds_from_lengths(lens, S) for lens in DOC_LENGTHS]
        ds = torch.stack([r[0] for r in rows]).cuda()
        de = torch.stack([r[1] for r in rows]).cuda()
    return slopes, window, table, ds, de


def _fwd_bwd(q, k, v, dout, scale, causal, vargs):
    o, lse = _ext().flash_fwd(q, k, v, scale, P_DROP, SEED, causal, None, *vargs)
    grads = _ext().flash_bwd(q, k, v, o, dout, lse, scale, P_DROP, SEED, causal,
                             None, None, *vargs)
    return (o, lse) + tuple(grads)


CASES = [("plain", True), ("plain", False), ("alibi", True), ("window", True),
         ("rel_bias", True), ("rel_bias", False), ("docs", True)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("variant,causal", CASES)
def test_strided_views_bit_equal_to_contiguous(variant, causal, d):
    q, k, v = _views(d)
    vargs = _variant_args(variant)
    scale = 1.0 / math.sqrt(d)
    dout = torch.randn(B, S, H, d, device="cuda", dtype=torch.bfloat16,
                       generator=torch.Generator(device="cuda").manual_seed(3))
    got = _fwd_bwd(q, k, v, dout, scale, causal, vargs)
    want = _fwd_bwd(q.contiguous(), k.contiguous(), v.contiguous(), dout, scale,
                    causal, vargs)
    assert len(got) == len(want) == (6 if variant == "rel_bias" else 5)
    assert got[2].shape == (B, S, H, d)
    assert got[3].shape == got[4].shape == (B, S, HKV, d)
    for name, a, b_ in zip(("o", "lse", "dq", "dk", "dv"), got, want):
        assert torch.equal(a, b_), f"{variant} d{d} causal{int(causal)}: {name} differs"
        assert a.float().abs().max().item() > 0, name
    if variant == "rel_bias":
        rel = _rel_err(got[5], want[5])
        print(f"[strides] d{d} causal{int(causal)} dtable rel diff {rel:.3e}")
        assert rel < GRAD_TOL and want[5].abs().max().item() > 0


def test_fwd_positional_matches_keyword():
    """Pins the pybind argument order: `window` sits at position 9."""
    d = 64
    q, k, v = _views(d)
    scale = 1.0 / math.sqrt(d)
    o1, lse1 = _ext().flash_fwd(q, k, v, scale, P_DROP, SEED, True, None, None,
                                WINDOW)
    o2, lse2 = _ext().flash_fwd(q=q, k=k, v=v, scale=scale, p_drop=P_DROP, seed=SEED,
                                causal=True, kv_len=None, alibi_slopes=None,
                                window=WINDOW)
    assert torch.equal(o1, o2) and torch.equal(lse1, lse2)
    # the window must matter at this shape, or the order is not pinned
    o0, _ = _ext().flash_fwd(q, k, v, scale, P_DROP, SEED, True, None)
    assert not torch.equal(o0, o1)
