"""Fused T5 relative-position bias in the flash-attention kernels vs an fp32
PyTorch reference whose bias is materialized in fp32 from the same table:
bias[h, i, j] = table[h, j - i + Sq - 1].  The table is learned, so every
backward case also checks its gradient (dS without the scale, summed along
diagonals and over the batch)."""

import math

import pytest
import torch

from tests.dropout_oracle import attn_keep_mask, keep_scale

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2    # max-abs (the project's bound vs fp32)
GRAD_TOL = 5e-2   # relative to the reference grad's max-abs

B, H = 2, 4
SEED = (1 << 61) + 0xDEADBEEF  # the kernels fold seed >> 32 into the key


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


def _table(h, sq, sk, seed=11, grad=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(h, sq + sk - 1, device="cuda", dtype=torch.float32,
                    generator=g) * 0.5
    return t.requires_grad_(grad)


def _materialize(table, sq, sk):
    """[H, Sq, Sk] fp32 bias from the [H, Sq + Sk - 1] table (differentiable)."""
    i = torch.arange(sq, device=table.device)[:, None]
    j = torch.arange(sk, device=table.device)[None, :]
    return table[:, j - i + (sq - 1)]


def _ref(q, k, v, scale, causal, table, kv_len=None, keep=None, ks=1.0):
    """fp32 reference on [B, S, H(q), D] / [B, S, Hkv, D] inputs; keep is the
    dropout keep mask [B, H, Sq, Sk] (bool) with its 1 / (1 - p) scale ks."""
    group = q.shape[2] // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    vh = v.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    sq, sk = s.shape[-2], s.shape[-1]
    s = s + _materialize(table, sq, sk)[None]
    if kv_len is not None:
        pad = (torch.arange(sk, device=q.device)[None, None, None, :]
               >= kv_len[:, None, None, None])
        s = s.masked_fill(pad, float("-inf"))
    if causal:
        cm = torch.ones(sq, sk, dtype=torch.bool, device=q.device).tril_(sk - sq)
        s = s.masked_fill(~cm, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep.to(p.dtype) * ks
    return torch.matmul(p, vh).permute(0, 2, 1, 3)


def _qkv(b, s, h, d, hkv=None, seed=0, grad=False):
    torch.manual_seed(seed)
    hkv = hkv or h
    mk = lambda n: torch.randn(b, s, n, d, device="cuda", dtype=torch.bfloat16,
                               requires_grad=grad)
    return mk(h), mk(hkv), mk(hkv)


def _rel_err(got, want):
    return ((got.float() - want.float()).abs().max()
            / (want.float().abs().max() + 1e-6)).item()


def _check_grads(pairs, tag):
    for name, got, want in pairs:
        rel = _rel_err(got, want)
        print(f"[relbias] {tag} {name} rel err {rel:.3e}")
        assert rel < GRAD_TOL, f"{tag} {name} rel err {rel}"


def _fwd_bwd_vs_ref(b, s, h, d, causal, hkv=None, kv_len=None, seed=0):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(b, s, h, d, hkv=hkv, seed=seed, grad=True)
    table = _table(h, s, s, grad=True)
    scale = 1.0 / math.sqrt(d)
    o = flash_attention(q, k, v, scale, p_drop=0.0, causal=causal, kv_len=kv_len,
                        rel_bias=table)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    tr = table.detach().clone().requires_grad_(True)
    ref = _ref(qr, kr, vr, scale, causal, tr, kv_len=kv_len)
    g = torch.randn_like(ref)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = (torch.arange(s, device="cuda")[None, :] < kv_len[:, None]).float()
        g = g * qmask[:, :, None, None]
    err = (o.float() - ref).abs().max().item()
    tag = f"s{s} d{d} causal{int(causal)} hkv{hkv or h}"
    print(f"[relbias] {tag} fwd max err {err:.3e}")
    assert err < FWD_TOL, f"relbias fwd max err {err}"
    o.backward(g.to(torch.bfloat16))
    ref.backward(g)
    assert table.grad.dtype == torch.float32 and table.grad.shape == table.shape
    _check_grads([("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                  ("dv", v.grad, vr.grad), ("dtable", table.grad, tr.grad)], tag)
    if causal:
        # no visible pair has kv > q: those diagonals are never touched
        assert (table.grad[:, s:] == 0).all()
        assert (tr.grad[:, s:] == 0).all()
    return q, k, v, table


# 1. forward -----------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s", [128, 200, 384])
def test_relbias_fwd_matches_reference(d, causal, s):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(B, s, H, d)
    table = _table(H, s, s)
    scale = 1.0 / math.sqrt(d)
    o = flash_attention(q, k, v, scale, p_drop=0.0, causal=causal, rel_bias=table)
    ref = _ref(q, k, v, scale, causal, table)
    err = (o.float() - ref).abs().max().item()
    print(f"[relbias] s{s} d{d} causal{int(causal)} fwd max err {err:.3e}")
    assert err < FWD_TOL, f"relbias fwd max err {err}"
    # the bias must matter at this shape, or the comparison shows nothing
    o_none = flash_attention(q, k, v, scale, p_drop=0.0, causal=causal)
    assert (o.float() - o_none.float()).abs().max().item() > FWD_TOL


# 2. forward + backward, dtable included -----------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s", [200, 384])
def test_relbias_backward_matches_reference(d, causal, s):
    # scale = 1/sqrt(d): a stray `scale` in dtable would be 8x or 11x off
    _fwd_bwd_vs_ref(B, s, H, d, causal=causal)


# 3. GQA: the table row belongs to the QUERY head --------------------------------
@pytest.mark.parametrize("hkv", [4, 2])
def test_relbias_gqa_matches_reference(hkv):
    _fwd_bwd_vs_ref(B, 256, 8, 64, causal=True, hkv=hkv, seed=2)


# 4. kv_len + table ----------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_relbias_kv_len_padding_matches_reference(causal):
    lens = torch.tensor([200, 136, 57, 1], device="cuda", dtype=torch.int32)
    s = 200
    _, k, v, _ = _fwd_bwd_vs_ref(4, s, H, 64, causal=causal, kv_len=lens, seed=1)
    kpad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert k.grad.float()[kpad].abs().max().item() == 0.0
    assert v.grad.float()[kpad].abs().max().item() == 0.0


# 5. dropout with the oracle's mask ---------------------------------------------------
_KEEP = {}


def _keep(s, p):
    """Oracle mask [B, H, S, S] on the device; computed once per key, read-only."""
    if (s, p) not in _KEEP:
        _KEEP[(s, p)] = attn_keep_mask(SEED, B * H, s, s, p).view(B, H, s, s).cuda()
    return _KEEP[(s, p)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_relbias_dropout_same_mask_matches_reference(d, causal, p):
    s = 200
    q, k, v = _qkv(B, s, H, d, seed=3)
    table = _table(H, s, s)
    scale = 1.0 / math.sqrt(d)
    o, lse = _ext().flash_fwd(q, k, v, scale, p, SEED, causal, None, None, 0, table)
    g = torch.randn(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    dq, dk, dv, dtab = _ext().flash_bwd(q, k, v, o, g, lse, scale, p, SEED, causal,
                                        None, None, None, 0, table)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    tr = table.clone().requires_grad_(True)
    ref = _ref(qr, kr, vr, scale, causal, tr, keep=_keep(s, p),
               ks=float(keep_scale(p)))
    tag = f"dropout p{p} d{d} causal{int(causal)}"
    err = (o.float() - ref).abs().max().item()
    print(f"[relbias] {tag} fwd max err {err:.3e} bound {FWD_TOL / (1 - p):.3e}")
    assert err < FWD_TOL / (1 - p), f"{tag} fwd max err {err}"
    ref.backward(g.float())
    _check_grads([("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad),
                  ("dtable", dtab, tr.grad)], tag)


# 6. tile-class invariance ---------------------------------------------------------------
def test_relbias_tile_class_invariance():
    """Non-causal S = 200 against the same tensors zero-padded to 224 with
    kv_len = 200: other tile classes, the same visible pairs."""
    s, sp, d = 200, 224, 64
    scale = 1.0 / math.sqrt(d)
    q, k, v = _qkv(B, s, H, d, seed=4)
    table = _table(H, s, s)
    g = torch.randn(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, 0, 0, sp - s))
    qp, kp, vp, gp = pad(q), pad(k), pad(v), pad(g)
    # diagonal delta sits at delta + Sq - 1: shift by the new offset
    tp = torch.zeros(H, 2 * sp - 1, device="cuda", dtype=torch.float32)
    tp[:, sp - s:sp - s + 2 * s - 1] = table
    lens = torch.full((B,), s, device="cuda", dtype=torch.int32)

    o, lse = _ext().flash_fwd(q, k, v, scale, 0.0, 0, False, None, None, 0, table)
    dq, dk, dv, dt = _ext().flash_bwd(q, k, v, o, g, lse, scale, 0.0, 0, False,
                                      None, None, None, 0, table)
    o2, lse2 = _ext().flash_fwd(qp, kp, vp, scale, 0.0, 0, False, lens, None, 0, tp)
    # padded query rows: zero upstream gradient (they never reach a loss)
    dq2, dk2, dv2, dt2 = _ext().flash_bwd(qp, kp, vp, o2, gp, lse2, scale, 0.0, 0,
                                          False, None, lens, None, 0, tp)
    assert torch.equal(o, o2[:, :s])
    assert torch.equal(lse, lse2[:, :, :s])
    assert torch.equal(dq, dq2[:, :s])
    assert torch.equal(dk, dk2[:, :s])
    assert torch.equal(dv, dv2[:, :s])
    # atomic summation order is not fixed: tolerance only
    rel = _rel_err(dt2[:, sp - s:sp - s + 2 * s - 1], dt)
    print(f"[relbias] tile-class dtable rel diff {rel:.3e}")
    assert rel < GRAD_TOL
    # diagonals only padded keys reach stay exactly zero
    assert (dt2[:, :sp - s] == 0).all() and (dt2[:, sp - s + 2 * s - 1:] == 0).all()


# 7. packed qkv path ----------------------------------------------------------------------
def test_relbias_qkv_packed_matches_view_path():
    from libai_amd.ops.attention import flash_attention, flash_attention_qkv

    torch.manual_seed(7)
    b, s, h, d = 2, 256, 4, 64
    qkv = torch.randn(b, s, h, 3, d, device="cuda", dtype=torch.bfloat16)
    q1 = qkv.clone().requires_grad_(True)
    q2 = qkv.clone().requires_grad_(True)
    t1 = _table(h, s, s, grad=True)
    t2 = _table(h, s, s, grad=True)
    o1 = flash_attention_qkv(q1, scale=d ** -0.5, p_drop=0.0, causal=True,
                             rel_bias=t1)
    o2 = flash_attention(q2[..., 0, :], q2[..., 1, :], q2[..., 2, :],
                         scale=d ** -0.5, p_drop=0.0, causal=True, rel_bias=t2)
    assert torch.equal(o1, o2)
    g = torch.randn_like(o1)
    o1.backward(g)
    o2.backward(g)
    assert torch.equal(q1.grad, q2.grad)
    rel = _rel_err(t1.grad, t2.grad)
    print(f"[relbias] packed vs views dtable rel diff {rel:.3e}")
    assert rel < GRAD_TOL and t1.grad.abs().max().item() > 0
    # a table that does not require grad gets none, and the call still works
    t3 = _table(h, s, s)
    q3 = qkv.clone().requires_grad_(True)
    o3 = flash_attention_qkv(q3, scale=d ** -0.5, p_drop=0.0, causal=True,
                             rel_bias=t3)
    o3.backward(g)
    assert t3.grad is None and torch.equal(q3.grad, q1.grad)


# 8. the bias is the only difference ---------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_relbias_zero_table_is_bit_equal_to_no_table(causal):
    s, d = 200, 64
    scale = 1.0 / math.sqrt(d)
    q, k, v = _qkv(B, s, H, d, seed=5)
    g = torch.randn(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    zeros = torch.zeros(H, 2 * s - 1, device="cuda", dtype=torch.float32)
    o0, lse0 = _ext().flash_fwd(q, k, v, scale, 0.0, 0, causal, None, None, 0)
    res0 = _ext().flash_bwd(q, k, v, o0, g, lse0, scale, 0.0, 0, causal, None, None,
                            None, 0)
    assert len(res0) == 3  # no table: the arity is unchanged
    o1, lse1 = _ext().flash_fwd(q, k, v, scale, 0.0, 0, causal, None, None, 0, zeros)
    res1 = _ext().flash_bwd(q, k, v, o1, g, lse1, scale, 0.0, 0, causal, None, None,
                            None, 0, zeros)
    assert len(res1) == 4
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    for a, b_ in zip(res0, res1[:3]):
        assert torch.equal(a, b_)


# 9. binding rejections ------------------------------------------------------------------------
def test_relbias_binding_rejections():
    s, d = 128, 64
    q, k, v = _qkv(B, s, H, d)
    good = _table(H, s, s)
    slopes = torch.ones(H, device="cuda", dtype=torch.float32)
    fwd = lambda t, sl=None, w=0: _ext().flash_fwd(q, k, v, 0.125, 0.0, 0, True, None,
                                                   sl, w, t)
    o, lse = fwd(good)
    bwd = lambda t, sl=None, w=0: _ext().flash_bwd(q, k, v, o, torch.ones_like(o), lse,
                                                   0.125, 0.0, 0, True, None, None,
                                                   sl, w, t)
    bad = {
        "dtype": (good.to(torch.bfloat16), None, 0),
        "shape": (torch.zeros(H, 2 * s, device="cuda"), None, 0),
        "non-contiguous": (torch.zeros(2 * s - 1, H, device="cuda").t(), None, 0),
        "table + slopes": (good, slopes, 0),
        "table + window": (good, None, 16),
    }
    for name, (t, sl, w) in bad.items():
        with pytest.raises(RuntimeError):
            fwd(t, sl, w)
        with pytest.raises(RuntimeError):
            bwd(t, sl, w)
