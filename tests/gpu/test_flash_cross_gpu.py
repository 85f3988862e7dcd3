"""Non-causal flash attention with Sq != Sk (cross-attention), forward and
backward, and the packed-kv entry point ``flash_attention_kv``."""

import math

import pytest
import torch

from tests.dropout_oracle import attn_keep_mask, keep_scale, ref_attention_masked

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2   # max abs vs fp32 (tests/gpu/test_flash_attn_gpu.py)
GRAD_TOL = 5e-2  # max-rel vs fp32 (same file)
B, H = 2, 4


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _inputs(sq, sk, d, hkv=H, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, sq, H, d, device="cuda", dtype=torch.bfloat16)
    kv5 = torch.randn(B, sk, hkv, 2, d, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(B, sq, H, d, device="cuda", dtype=torch.bfloat16)
    return q, kv5, g


def _rel(got, want):
    return ((got.float() - want).abs().max() / (want.abs().max() + 1e-6)).item()


def _reference(q, k, v, g, scale, kv_len=None, keep=None, ks=1.0):
    """fp32 O, dq, dk, dv (the oracle's masked attention, all-ones keep mask
    without dropout)."""
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    if keep is None:
        keep = torch.ones(B, H, q.shape[1], k.shape[1], device=q.device)
    o = ref_attention_masked(qr, kr, vr, scale, keep, ks, causal=False, kv_len=kv_len)
    o.backward(g.float())
    return o.detach(), qr.grad, kr.grad, vr.grad


def _check_all(tag, got, want):
    o, dq, dk, dv = got
    ro, rdq, rdk, rdv = want
    err = (o.float() - ro).abs().max().item()
    print(f"[flash-cross] {tag} O max abs err {err:.3e}")
    assert err < FWD_TOL, f"{tag}: O max abs err {err}"
    for name, a, b in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        e = _rel(a, b)
        print(f"[flash-cross] {tag} {name} rel err {e:.3e}")
        assert e < GRAD_TOL, f"{tag}: {name} rel err {e}"


def _run_separate(q, kv5, g, scale, **kw):
    from libai_amd.ops.attention import flash_attention

    q = q.detach().requires_grad_(True)
    k = kv5[..., 0, :].detach().requires_grad_(True)
    v = kv5[..., 1, :].detach().requires_grad_(True)
    o = flash_attention(q, k, v, scale, causal=False, **kw)
    o.backward(g)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("sq,sk,kv_len", [(40, 200, None), (136, 64, None),
                                          (200, 328, [328, 203])])
def test_cross_fwd_bwd_matches_reference(d, sq, sk, kv_len):
    q, kv5, g = _inputs(sq, sk, d)
    scale = 1.0 / math.sqrt(d)
    if kv_len is not None:
        kv_len = torch.tensor(kv_len, device="cuda", dtype=torch.int32)
    got = _run_separate(q, kv5, g, scale, kv_len=kv_len)
    want = _reference(q, kv5[..., 0, :], kv5[..., 1, :], g, scale, kv_len=kv_len)
    _check_all(f"d{d} {sq}x{sk}", got, want)
    if kv_len is not None:  # padded keys get exact zero gradients
        assert got[2][1, 203:].abs().max().item() == 0
        assert got[3][1, 203:].abs().max().item() == 0


@pytest.mark.parametrize("d", [64, 128])
def test_cross_gqa_matches_reference(d):
    sq, sk = 136, 200
    q, kv5, g = _inputs(sq, sk, d, hkv=1)
    scale = 1.0 / math.sqrt(d)
    got = _run_separate(q, kv5, g, scale)
    want = _reference(q, kv5[..., 0, :], kv5[..., 1, :], g, scale)
    _check_all(f"gqa d{d}", got, want)


@pytest.mark.parametrize("d", [64, 128])
def test_cross_dropout_matches_same_mask_reference(d):
    from libai_amd.ops._ext import ext

    sq, sk, p, seed = 136, 200, 0.1, (1 << 61) + 0xDEADBEEF
    q, kv5, g = _inputs(sq, sk, d)
    k, v = kv5[..., 0, :], kv5[..., 1, :]
    scale = 1.0 / math.sqrt(d)
    o, lse = ext().flash_fwd(q, k, v, scale, p, seed, False, None)
    dq, dk, dv = ext().flash_bwd(q, k, v, o, g, lse, scale, p, seed, False, None,
                                 None)
    keep = attn_keep_mask(seed, B * H, sq, sk, p).view(B, H, sq, sk).cuda()
    want = _reference(q, k, v, g, scale, keep=keep, ks=keep_scale(p))
    _check_all(f"dropout d{d}", (o, dq, dk, dv), want)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("padded", [False, True])
def test_packed_kv_equals_separate_views(d, padded):
    from libai_amd.ops.attention import flash_attention_kv

    sq, sk = 136, 200
    q, kv5, g = _inputs(sq, sk, d, seed=1)
    scale = 1.0 / math.sqrt(d)
    kv_len = (torch.tensor([200, 77], device="cuda", dtype=torch.int32)
              if padded else None)
    o_s, dq_s, dk_s, dv_s = _run_separate(q, kv5, g, scale, kv_len=kv_len)
    qp = q.detach().requires_grad_(True)
    kvp = kv5.detach().requires_grad_(True)
    o = flash_attention_kv(qp, kvp, scale, kv_len=kv_len)
    o.backward(g)
    assert torch.equal(o, o_s)
    assert torch.equal(qp.grad, dq_s)
    assert kvp.grad.shape == kv5.shape
    assert torch.equal(kvp.grad[..., 0, :], dk_s)
    assert torch.equal(kvp.grad[..., 1, :], dv_s)
