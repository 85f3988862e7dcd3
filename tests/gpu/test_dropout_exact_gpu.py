"""Same-mask dropout tests: every dropout kernel rebuilds its mask in the
backward pass, so each one is compared value by value, and gradient by
gradient, with an fp32 reference that applies the SAME mask.

The attention and bias masks come from tests/dropout_oracle.py, a numpy
re-statement of the hash that shares no code with the kernels; the fused
softmax (philox) mask is recovered from the forward output.  Also here: the
bias ops at widths that are no multiple of the vector width, and colsum.

Every test prints the error it measured next to its bound
("[dropout-exact] ...") before it asserts.
"""

import math

import pytest
import torch

from tests.dropout_oracle import (attn_keep_mask, elem_keep_mask, keep_rate,
                                  keep_scale, ref_attention_masked,
                                  ref_attention_probs)

pytestmark = pytest.mark.gpu

# the project's bounds for the same comparisons at p = 0
FWD_TOL = 2e-2    # max-abs; times 1 / (1 - p): P and O are rounded to bf16
#                   after the 1 / (1 - p) scale, nothing else changes
GRAD_TOL = 5e-2   # relative to the reference grad's max-abs (scale cancels)

B, H = 2, 4
SEED_LO = 0x1234567
SEED_HI = (1 << 61) + 0xDEADBEEF  # the kernels fold seed >> 32 into the key


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


def _report(group, tag, name, err, bound):
    print(f"[dropout-exact] {group} | {tag} | {name} err {err:.3e} bound {bound:.3e}")


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


# ===========================================================================
# attention
# ===========================================================================
_KEEP = {}


def _keep(seed, s, p):
    """Oracle mask [B, H, S, S] on the device; computed once per key, read-only."""
    key = (seed, s, p)
    if key not in _KEEP:
        _KEEP[key] = attn_keep_mask(seed, B * H, s, s, p).view(B, H, s, s).cuda()
    return _KEEP[key]


def _qkv(s, d, hkv=None, seed=0):
    torch.manual_seed(seed)
    hkv = hkv or H
    mk = lambda n: torch.randn(B, s, n, d, device="cuda", dtype=torch.bfloat16)
    return mk(H), mk(hkv), mk(hkv)


def _onehot_block(s, d, c):
    """[B, S, H, D] bf16: row r of block c (c*D <= r < (c+1)*D) holds the
    one-hot vector of r - c*D, every other row is zero."""
    t = torch.zeros(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    r = torch.arange(c * d, min((c + 1) * d, s), device="cuda")
    t[:, r, :, r - c * d] = 1
    return t


# 1. attn_dropout_apply == oracle ------------------------------------------------
@pytest.mark.parametrize("seed", [SEED_LO, SEED_HI])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("s", [64, 200, 384])
def test_attn_dropout_apply_is_the_oracle_mask(s, p, seed):
    want = _keep(seed, s, p).view(B * H, s, s).float() * float(keep_scale(p))
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.ones(B * H, s, s, device="cuda", dtype=dtype)
        _ext().attn_dropout_apply(x, s, s, p, seed)
        assert torch.equal(x, want.to(dtype)), f"{dtype} mask differs from the oracle"


def _check_dropped_probs(pd, p_ref, keep, p, group, tag):
    """pd: the kernel's dropped probabilities [B, H, S, S] (bf16 values in
    fp32).  Mask equality wherever the fp32 probability is representable,
    exact zeros on masked entries, and kept values within bf16 rounding of
    P / (1 - p)."""
    live = p_ref > 1e-30
    got_keep = pd != 0
    wrong = (got_keep != keep) & live
    assert not wrong.any(), (
        f"{tag}: {int(wrong.sum())} mask entries differ from the oracle, first at "
        f"{wrong.nonzero()[0].tolist()}")
    assert (pd[p_ref == 0] == 0).all(), f"{tag}: masked entry is non-zero"
    want = p_ref * float(keep_scale(p))
    sel = live & keep
    err = (pd - want).abs()[sel]
    bound = 2.0 ** -7 * want[sel] + FWD_TOL / (1 - p)
    _report(group, tag, "Pd max-abs", err.max().item(), FWD_TOL / (1 - p))
    _report(group, tag, "Pd max of err / (2^-7 * ref + fwd bound)",
            (err / bound).max().item(), 1.0)
    assert (err <= bound).all(), f"{tag}: kept value off by {err.max().item()}"


_EXACT = [(d, s, causal, p) for d in (64, 128) for s in (64, 200, 384)
          for causal in (True, False) for p in (0.1, 0.5)]


# 2. forward mask, exact -------------------------------------------------------------
@pytest.mark.parametrize("d,s,causal,p", _EXACT)
def test_flash_fwd_mask_is_the_oracle_mask(d, s, causal, p):
    """With V a one-hot block over the key index, O is a block of the dropped
    probability matrix; ceil(S / D) forwards give all of it."""
    seed = SEED_HI
    q, k, _ = _qkv(s, d, seed=1)
    scale = 1.0 / math.sqrt(d)
    _, lse0 = _ext().flash_fwd(q, k, _onehot_block(s, d, 0), scale, 0.0, 0, causal,
                               None, None, 0)
    cols = []
    for c in range((s + d - 1) // d):
        o, lse = _ext().flash_fwd(q, k, _onehot_block(s, d, c), scale, p, seed,
                                  causal, None, None, 0)
        assert torch.equal(lse, lse0), "dropout must not touch the logsumexp"
        cols.append(o)  # o[b, i, h, dd] = Pd[b, h, i, c*D + dd]
    pd = torch.cat(cols, dim=3)[..., :s].permute(0, 2, 1, 3).float()
    p_ref = ref_attention_probs(q, k, scale, causal)
    _check_dropped_probs(pd, p_ref, _keep(seed, s, p), p, "fwd mask",
                         f"d{d} s{s} causal{int(causal)} p{p}")


# 3. dV-path mask, exact ---------------------------------------------------------------
@pytest.mark.parametrize("d,s,causal,p", _EXACT)
def test_flash_bwd_kv_mask_is_the_oracle_mask(d, s, causal, p):
    """With dO a one-hot block over the query index, dV is a block of the
    dropped probability matrix as the dK/dV kernel regenerates it (one hash
    per lane of a quad, redistributed by DPP)."""
    seed = SEED_HI
    q, k, v = _qkv(s, d, seed=2)
    scale = 1.0 / math.sqrt(d)
    o, lse = _ext().flash_fwd(q, k, v, scale, p, seed, causal, None, None, 0)
    rows = []
    for c in range((s + d - 1) // d):
        _, _, dv = _ext().flash_bwd(q, k, v, o, _onehot_block(s, d, c), lse, scale,
                                    p, seed, causal, None, None, None, 0)
        rows.append(dv)  # dv[b, j, h, dd] = Pd[b, h, c*D + dd, j]
    pd = torch.cat(rows, dim=3)[..., :s].permute(0, 2, 3, 1).float()
    p_ref = ref_attention_probs(q, k, scale, causal)
    _check_dropped_probs(pd, p_ref, _keep(seed, s, p), p, "dV-path mask",
                         f"d{d} s{s} causal{int(causal)} p{p}")


# 4. forward and dq/dk/dv vs the masked reference -----------------------------------------
def _zero_ref_bound(q, k, v, g, scale, p):
    """With window = 1 every row's softmax is over ONE key: P = 1 and the exact
    dS = P * (keep * dO.V^T - rowsum(dO * O)) is 0, so the reference dQ and dK
    are identically zero and "relative to the reference's max-abs" has no
    scale.  The kernels form the two terms separately:
    * as fp32 dot products of D bf16 products summed in different orders, each
      within D * 2^-24 * sum|terms| <= D^2 * 2^-24 * max|dO| * max|V| / (1-p);
    * from O = bf16(V / (1 - p)), rounded by up to 2^-9 relative per element
      (exact at p = 0.5), which moves rowsum(dO * O) by at most
      D * 2^-9 * max|dO| * max|V| / (1 - p).
    dQ/dK multiply the difference by scale * K (or Q)."""
    d = q.shape[-1]
    amax = lambda t: t.detach().float().abs().max().item()
    ks = float(keep_scale(p))
    dot_err = d * d * 2.0 ** -24 * amax(g) * amax(v) * ks
    o_round = d * 2.0 ** -9 * amax(g) * amax(v) * ks
    return (2.0 * dot_err + o_round) * scale * max(amax(q), amax(k))


def _slopes():
    from libai_amd.layers.position_bias import alibi_slopes

    return alibi_slopes(H).to(device="cuda", dtype=torch.float32).contiguous()


def _fwd_bwd_vs_oracle(group, s, d, p, causal, hkv=None, kv_len=None, alibi=False,
                       window=0, seed=SEED_HI, data_seed=3):
    q, k, v = _qkv(s, d, hkv=hkv, seed=data_seed)
    scale = 1.0 / math.sqrt(d)
    slopes = _slopes() if alibi else None
    tag = (f"d{d} s{s} causal{int(causal)} p{p} hkv{hkv or H} "
           f"kvlen{int(kv_len is not None)} alibi{int(alibi)} w{window}")

    o, lse = _ext().flash_fwd(q, k, v, scale, p, seed, causal, kv_len, slopes, window)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = ref_attention_masked(qr, kr, vr, scale, _keep(seed, s, p), keep_scale(p),
                               causal, kv_len=kv_len, alibi_slopes=slopes,
                               window=window)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - ref).abs().max().item()
    _report(group, tag, "fwd max-abs", err, FWD_TOL / (1 - p))

    g = torch.randn(B, s, H, d, device="cuda").to(torch.bfloat16)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = torch.arange(s, device="cuda")[None, :] < kv_len[:, None]
        g = g * qmask[:, :, None, None].to(g.dtype)
    dq, dk, dv = _ext().flash_bwd(q, k, v, o, g, lse, scale, p, seed, causal, None,
                                  kv_len, slopes, window)
    ref.backward(g.float())
    failures = []
    if not err < FWD_TOL / (1 - p):
        failures.append(f"fwd max-abs {err}")
    zero_bound = _zero_ref_bound(q, k, v, g, scale, p)
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad),
                            ("dv", dv, vr.grad)):
        assert torch.isfinite(got.float()).all(), f"{tag} {name} not finite"
        aerr = (got.float() - want).abs().max().item()
        if want.abs().max().item() == 0.0:
            _report(group, tag, f"{name} max-abs (zero reference)", aerr, zero_bound)
            if not aerr < zero_bound:
                failures.append(f"{name} abs {aerr} (zero reference)")
            continue
        rel = aerr / (want.abs().max().item() + 1e-6)
        _report(group, tag, f"{name} rel", rel, GRAD_TOL)
        if not rel < GRAD_TOL:
            failures.append(f"{name} rel {rel}")
    assert not failures, f"{tag}: " + ", ".join(failures)
    return q, k, v, o, dq, dk, dv


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s", [200, 384])
@pytest.mark.parametrize("d", [64, 128])
def test_flash_dropout_matches_masked_reference(d, s, causal, p):
    _fwd_bwd_vs_oracle("attention", s, d, p, causal)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("hkv", [1, 2])
@pytest.mark.parametrize("d", [64, 128])
def test_flash_dropout_gqa_matches_masked_reference(d, hkv, p):
    """The dK/dV kernel runs on a B * Hkv grid and must key the mask on the
    QUERY head of each group member."""
    _fwd_bwd_vs_oracle("attention gqa", 200, d, p, True, hkv=hkv, data_seed=4)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("d", [64, 128])
def test_flash_dropout_kv_len_matches_masked_reference(d, causal, p):
    s = 200
    lens = torch.tensor([s, s - 37], device="cuda", dtype=torch.int32)
    _, _, _, _, _, dk, dv = _fwd_bwd_vs_oracle("attention kv_len", s, d, p, causal,
                                               kv_len=lens, data_seed=5)
    pad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert dk.float()[pad].abs().max().item() == 0.0
    assert dv.float()[pad].abs().max().item() == 0.0


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("d", [64, 128])
def test_flash_dropout_alibi_matches_masked_reference(d, causal, p):
    _fwd_bwd_vs_oracle("attention alibi", 200, d, p, causal, alibi=True, data_seed=6)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("window", [1, 65, 129])
@pytest.mark.parametrize("d", [64, 128])
def test_flash_dropout_window_matches_masked_reference(d, window, p):
    _fwd_bwd_vs_oracle("attention window", 384, d, p, True, window=window,
                       data_seed=7)


@pytest.mark.parametrize("d", [64, 128])
def test_flash_dropout_packed_dqkv_equals_view_path(d):
    """The packed [B, S, H, 3, D] gradient buffer gets bit-for-bit the
    gradients of the separate-tensor path at the same seed, and strided q/k/v
    views give bit-for-bit the output of contiguous copies."""
    s, p, seed = 200, 0.1, SEED_HI
    torch.manual_seed(8)
    qkv = torch.randn(B, s, H, 3, d, device="cuda", dtype=torch.bfloat16)
    q, k, v = qkv[..., 0, :], qkv[..., 1, :], qkv[..., 2, :]
    scale = d ** -0.5
    o, lse = _ext().flash_fwd(q, k, v, scale, p, seed, True, None, None, 0)
    o_c, lse_c = _ext().flash_fwd(q.contiguous(), k.contiguous(), v.contiguous(),
                                  scale, p, seed, True, None, None, 0)
    assert torch.equal(o, o_c) and torch.equal(lse, lse_c)
    g = torch.randn(B, s, H, d, device="cuda").to(torch.bfloat16)
    dq, dk, dv = _ext().flash_bwd(q, k, v, o, g, lse, scale, p, seed, True, None,
                                  None, None, 0)
    dqkv = torch.full_like(qkv, float("nan"))
    _ext().flash_bwd(q, k, v, o, g, lse, scale, p, seed, True, dqkv, None, None, 0)
    assert torch.equal(dqkv[..., 0, :], dq)
    assert torch.equal(dqkv[..., 1, :], dk)
    assert torch.equal(dqkv[..., 2, :], dv)
    # and those gradients are the right ones
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = ref_attention_masked(qr, kr, vr, scale, _keep(seed, s, p), keep_scale(p),
                               True)
    ref.backward(g.float())
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad),
                            ("dv", dv, vr.grad)):
        rel = _rel_err(got, want)
        _report("attention packed", f"d{d} s{s}", f"{name} rel", rel, GRAD_TOL)
        assert rel < GRAD_TOL


# ===========================================================================
# fused scale + mask + softmax (+ dropout)
# ===========================================================================
def _softmax_ref(sr, mask, scale, causal):
    sq, sk = sr.shape[-2], sr.shape[-1]
    sf = sr * scale
    if causal:
        cm = torch.ones(sq, sk, dtype=torch.bool, device=sr.device).tril_(sk - sq)
        sf = sf.masked_fill(~cm, float("-inf"))
    if mask is not None:
        sf = sf - 10000.0 * mask[:, None, :, :].float()
    return torch.softmax(sf, dim=-1)


# the smallest shapes that reach each path of the kernel (b=1, nh=2):
# one vector per thread in a 64-thread block / a pad mask at an odd row count
# / nvec = 65 (bf16) or 130 (fp32), no multiple of the block, so the
# `iv >= nvec` break is taken / 2..4 vectors per thread / the 1024-thread
# block at the widest row the wrapper admits
_SOFTMAX_SHAPES = [(64, 64, True, False), (33, 96, False, True),
                   (8, 520, True, False), (8, 2048, True, False),
                   (4, 8192, False, False)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("sq,sk,causal,pad", _SOFTMAX_SHAPES)
def test_fused_softmax_dropout_matches_same_mask_reference(sq, sk, causal, pad, p,
                                                           dtype):
    from libai_amd.ops.softmax import fused_scale_mask_softmax

    torch.manual_seed(0)
    b, nh = 1, 2
    s = torch.randn(b, nh, sq, sk, device="cuda", dtype=dtype, requires_grad=True)
    mask = None
    if pad:
        mask = (torch.rand(b, sq, sk, device="cuda") < 0.2).to(torch.uint8)
    scale = 0.125
    y = fused_scale_mask_softmax(s, pad_mask=mask, scale=scale, p=p, causal=causal)
    assert y.dtype == dtype and torch.isfinite(y.float()).all()

    sr = s.detach().float().requires_grad_(True)
    pr = _softmax_ref(sr, mask, scale, causal)
    tag = f"sq{sq} sk{sk} causal{int(causal)} pad{int(pad)} p{p} {dtype}"
    if p > 0:
        live = pr.detach() > 1e-30
        keep = torch.where(live, y.detach() != 0, torch.ones_like(live))
        yr = pr * keep.float() * float(keep_scale(p))
        # the recovered mask is a dropout mask: keep rate 1 - p (philox
        # uniform > p) within 5 sigma
        n = int(live.sum())
        rate = keep[live].float().mean().item()
        sigma = math.sqrt(p * (1 - p) / n)
        _report("softmax", tag, "keep rate - (1-p)", abs(rate - (1 - p)), 5 * sigma)
        assert abs(rate - (1 - p)) < 5 * sigma
    else:
        yr = pr
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    err = _rel_err(y, yr)
    _report("softmax", tag, "y rel", err, tol)

    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float())
    gerr = _rel_err(s.grad, sr.grad)
    _report("softmax", tag, "ds rel", gerr, 3 * tol)
    assert err < tol and gerr < 3 * tol, f"{tag}: y {err}, ds {gerr}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_softmax_row_with_every_key_masked(dtype):
    """A pad mask that covers every key of a row adds -10000 to all of it: the
    row stays a softmax (no NaN).  Row 7 has constant scores, so it is exactly
    uniform.  Row 5 has random scores: at 10000 an fp32 score is quantised to
    2^-10, the kernel (one fused multiply-add) and the reference (multiply,
    then subtract) may round a score to different neighbours, which moves a
    probability by up to e^(2^-10) - 1 and the row sum by as much; that row is
    held to 2^-9 relative on top of the usual bound."""
    from libai_amd.ops.softmax import fused_scale_mask_softmax

    torch.manual_seed(0)
    b, nh, sq, sk = 1, 2, 33, 96
    s0 = torch.randn(b, nh, sq, sk, device="cuda", dtype=dtype)
    s0[:, :, 7, :] = 0.5
    s = s0.clone().requires_grad_(True)
    mask = (torch.rand(b, sq, sk, device="cuda") < 0.2).to(torch.uint8)
    mask[:, 5, :] = 1
    mask[:, 7, :] = 1
    y = fused_scale_mask_softmax(s, pad_mask=mask, scale=0.125, p=0.0, causal=False)
    assert torch.isfinite(y.float()).all()

    sr = s.detach().float().requires_grad_(True)
    yr = _softmax_ref(sr, mask, 0.125, False)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    amax = yr.abs().max().item()
    err = (y.float() - yr).abs()
    others = torch.ones(sq, dtype=torch.bool, device="cuda")
    others[5] = False
    e_other = err[:, :, others].max().item() / amax
    _report("softmax", f"all-masked row {dtype}", "other rows rel", e_other, tol)
    assert e_other < tol
    assert (yr[:, :, 7] - 1.0 / sk).abs().max().item() < 1e-7  # the uniform row
    ratio = (err[:, :, 5] / (2.0 ** -9 * yr[:, :, 5] + tol * amax)).max().item()
    _report("softmax", f"all-masked row {dtype}", "row 5 err / its bound", ratio, 1.0)
    assert ratio <= 1.0

    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float())
    assert torch.isfinite(s.grad.float()).all()
    gamax = sr.grad.abs().max().item()
    gerr = (s.grad.float() - sr.grad).abs()[:, :, others].max().item() / gamax
    _report("softmax", f"all-masked row {dtype}", "ds other rows rel", gerr, 3 * tol)
    assert gerr < 3 * tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sq,sk,causal", [(4, 8200, False), (8, 100, True)])
def test_fused_softmax_unsupported_widths_take_the_composed_path(monkeypatch, sq, sk,
                                                                 causal, dtype):
    from libai_amd.ops.softmax import fused_scale_mask_softmax

    calls = []
    for name in ("softmax_fwd", "softmax_bwd"):
        orig = getattr(_ext(), name)
        monkeypatch.setattr(_ext(), name,
                            lambda *a, _o=orig, **kw: (calls.append(1), _o(*a, **kw))[1])
    torch.manual_seed(0)
    s = torch.randn(1, 2, sq, sk, device="cuda", dtype=dtype, requires_grad=True)
    y = fused_scale_mask_softmax(s, scale=0.125, p=0.0, causal=causal)
    sr = s.detach().float().requires_grad_(True)
    yr = _softmax_ref(sr, None, 0.125, causal)
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float())
    assert calls == [], "the kernel ran on a width it does not serve"
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    err, gerr = _rel_err(y, yr), _rel_err(s.grad, sr.grad)
    _report("softmax composed", f"sk{sk} {dtype}", "y rel", err, tol)
    _report("softmax composed", f"sk{sk} {dtype}", "ds rel", gerr, 3 * tol)
    assert err < tol and gerr < 3 * tol
    # control: a served width does reach the kernel
    s2 = torch.randn(1, 2, 8, 128, device="cuda", dtype=dtype)
    fused_scale_mask_softmax(s2, scale=0.125, p=0.0, causal=True)
    assert calls == [1]


# ===========================================================================
# bias + dropout + residual
# ===========================================================================
# [5000, 64]: more rows than the 4096-block y grid, so the row-stride loop
# runs; [64, 1024]: several vector columns per block
_BIAS_SHAPES = [(5000, 64), (64, 1024)]


@pytest.mark.parametrize("seed", [SEED_LO, SEED_HI])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", _BIAS_SHAPES)
def test_bias_dropout_mask_is_the_oracle_mask(shape, p, seed):
    R, W = shape
    keep = elem_keep_mask(seed, R * W, p).view(R, W).cuda()
    ks = float(keep_scale(p))
    want = keep.float() * ks
    want_db = (keep.double() * ks).sum(0)
    kept = []
    for dtype in (torch.float32, torch.bfloat16):
        ones = torch.ones(R, W, device="cuda", dtype=dtype)
        y = _ext().bias_dropout_res_fwd(ones, None, None, p, seed)
        assert torch.equal(y, want.to(dtype)), f"fwd {dtype} differs from the oracle"
        dx, db = _ext().bias_dropout_res_bwd(ones, p, seed, True)
        assert torch.equal(dx, want.to(dtype)), f"bwd {dtype} differs from the oracle"
        tol = 1e-5 if dtype == torch.float32 else 2e-2
        err = _rel_err(db.double(), want_db)
        _report("bias dropout", f"{shape} p{p} {dtype}", "db_partial colsum rel", err,
                tol)
        assert err < tol
        dx2, db2 = _ext().bias_dropout_res_bwd(ones, p, seed, False)
        assert db2 is None and torch.equal(dx2, dx)
        kept.append(y != 0)
    assert torch.equal(kept[0], kept[1]), "bf16 and fp32 masks differ"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", _BIAS_SHAPES)
def test_bias_dropout_add_values_and_grads(shape, p, dtype):
    from libai_amd.ops._ext import draw_seed
    from libai_amd.ops.fused_bias import bias_dropout_add

    R, W = shape
    torch.manual_seed(1)
    x = torch.randn(R, W, device="cuda", dtype=dtype, requires_grad=True)
    b = torch.randn(W, device="cuda", dtype=dtype, requires_grad=True)
    r = torch.randn(R, W, device="cuda", dtype=dtype, requires_grad=True)
    dy = torch.randn(R, W, device="cuda", dtype=dtype)
    # the wrapper draws its seed from the CPU generator: replay the draw
    torch.manual_seed(11)
    seed = draw_seed()
    torch.manual_seed(11)
    y = bias_dropout_add(x, b, r, p=p, training=True)
    y.backward(dy)

    if p > 0:
        keep = elem_keep_mask(seed, R * W, p).view(R, W).cuda().float()
    else:
        keep = torch.ones(R, W, device="cuda")
    ks = float(keep_scale(p))
    y_ref = r.detach().float() + (x.detach().float() + b.detach().float()) * keep * ks
    dx_ref = dy.float() * keep * ks
    db_ref = dx_ref.double().sum(0)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    tag = f"{shape} p{p} {dtype}"
    errs = {"y": (_rel_err(y, y_ref), tol), "dx": (_rel_err(x.grad, dx_ref), 3 * tol),
            "dbias": (_rel_err(b.grad.double(), db_ref), 3 * tol)}
    for name, (e, bound) in errs.items():
        _report("bias dropout", tag, f"{name} rel", e, bound)
    assert all(e < bound for e, bound in errs.values()), f"{tag}: {errs}"
    assert torch.equal(r.grad, dy), "the residual gradient is dy itself"
    if p == 0:
        assert torch.equal(x.grad, dy), "without dropout dx is dy itself"
    else:
        # the kept set is exactly the oracle's, in the forward and the backward
        assert torch.equal(x.grad != 0, (keep != 0) & (dy != 0))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_bias_dropout_keep_rate_and_mean_scale(p):
    """The keep rate is (256 - thr8) / 256 while kept values are scaled by the
    unquantised 1 / (1 - p): the mean of keep / (1 - p) is their product, not
    1 (0.9983 at p = 0.1)."""
    R, W = 4096, 1024
    ones = torch.ones(R, W, device="cuda", dtype=torch.float32)
    y = _ext().bias_dropout_res_fwd(ones, None, None, p, SEED_LO)
    k = keep_rate(p)
    sigma = math.sqrt(k * (1 - k) / (R * W))
    rate = (y != 0).double().mean().item()
    _report("bias dropout", f"p{p}", "keep rate - (256-thr8)/256", abs(rate - k),
            5 * sigma)
    assert abs(rate - k) < 5 * sigma
    mean = y.double().mean().item()
    want = k / (1 - p)
    print(f"[dropout-exact] bias dropout | p{p} | mean of keep/(1-p) {mean:.6f} "
          f"expected {want:.6f}")
    assert abs(mean - want) < 5 * sigma / (1 - p)


# ===========================================================================
# widths that are no multiple of the vector width
# ===========================================================================
_RAGGED = [36, 31, 4]


def _forbid_kernels(monkeypatch, names):
    def boom(*a, **kw):
        raise AssertionError("a bias kernel was launched on a ragged width")

    for name in names:
        monkeypatch.setattr(_ext(), name, boom)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W", _RAGGED)
def test_bias_gelu_ragged_width(monkeypatch, W, dtype):
    from libai_amd.ops.fused_bias import bias_gelu

    _forbid_kernels(monkeypatch, ("bias_gelu_fwd", "bias_gelu_bwd"))
    torch.manual_seed(0)
    x = torch.randn(33, W, device="cuda", dtype=dtype, requires_grad=True)
    b = torch.randn(W, device="cuda", dtype=dtype, requires_grad=True)
    y = bias_gelu(x, b)
    assert y.shape == x.shape and torch.isfinite(y.float()).all()
    xr = x.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    yr = torch.nn.functional.gelu(xr + br)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g.float())
    errs = {"y": (_rel_err(y, yr), tol), "dx": (_rel_err(x.grad, xr.grad), 3 * tol),
            "dbias": (_rel_err(b.grad, br.grad), 3 * tol)}
    for name, (e, bound) in errs.items():
        _report("ragged bias_gelu", f"W{W} {dtype}", f"{name} rel", e, bound)
    assert all(e < bound for e, bound in errs.values()), errs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W", _RAGGED)
def test_bias_dropout_add_ragged_width(monkeypatch, W, dtype):
    from libai_amd.ops.fused_bias import bias_dropout_add

    _forbid_kernels(monkeypatch, ("bias_dropout_res_fwd", "bias_dropout_res_bwd"))
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    torch.manual_seed(0)
    x = torch.randn(33, W, device="cuda", dtype=dtype, requires_grad=True)
    b = torch.randn(W, device="cuda", dtype=dtype, requires_grad=True)
    r = torch.randn(33, W, device="cuda", dtype=dtype, requires_grad=True)
    dy = torch.randn(33, W, device="cuda", dtype=dtype)

    # p = 0: against the reference
    y = bias_dropout_add(x, b, r, p=0.0, training=True)
    y.backward(dy)
    y_ref = x.detach().float() + b.detach().float() + r.detach().float()
    errs = {"y": (_rel_err(y, y_ref), tol), "dx": (_rel_err(x.grad, dy), 3 * tol),
            "dbias": (_rel_err(b.grad, dy.float().sum(0)), 3 * tol),
            "dres": (_rel_err(r.grad, dy), 3 * tol)}
    for name, (e, bound) in errs.items():
        _report("ragged bias_dropout_add", f"W{W} {dtype} p0", f"{name} rel", e, bound)
    assert all(e < bound for e, bound in errs.values()), errs

    # p = 0.5: keep rate and the scale of the kept values (torch's own mask)
    p = 0.5
    x.grad = b.grad = None
    y = bias_dropout_add(x, b, None, p=p, training=True)
    y.backward(dy)
    keep = y.detach() != 0
    n = keep.numel()
    rate = keep.float().mean().item()
    sigma = math.sqrt(p * (1 - p) / n)
    _report("ragged bias_dropout_add", f"W{W} {dtype} p0.5", "keep rate - 0.5",
            abs(rate - (1 - p)), 5 * sigma)
    assert abs(rate - (1 - p)) < 5 * sigma
    y_ref = (x.detach().float() + b.detach().float()) * keep.float() / (1 - p)
    dx_ref = dy.float() * keep.float() / (1 - p)
    errs = {"y": (_rel_err(y, y_ref), tol), "dx": (_rel_err(x.grad, dx_ref), 3 * tol),
            "dbias": (_rel_err(b.grad, dx_ref.sum(0)), 3 * tol)}
    for name, (e, bound) in errs.items():
        _report("ragged bias_dropout_add", f"W{W} {dtype} p0.5", f"{name} rel", e,
                bound)
    assert all(e < bound for e, bound in errs.values()), errs


def test_bias_bindings_reject_ragged_widths():
    """The kernels index rows in whole vectors: the bindings refuse a width
    that is no multiple of the vector width (36 for bf16) or is smaller than
    one vector."""
    for W, dtype in ((36, torch.bfloat16), (4, torch.bfloat16), (31, torch.float32)):
        x = torch.randn(33, W, device="cuda", dtype=dtype)
        with pytest.raises(RuntimeError, match="width"):
            _ext().bias_gelu_fwd(x, None)
        with pytest.raises(RuntimeError, match="width"):
            _ext().bias_gelu_bwd(x, None, x, False)
        with pytest.raises(RuntimeError, match="width"):
            _ext().bias_dropout_res_fwd(x, None, None, 0.5, 1)
        with pytest.raises(RuntimeError, match="width"):
            _ext().bias_dropout_res_bwd(x, 0.5, 1, False)


def test_bias_bindings_serve_fp32_width_36():
    """36 is a multiple of the fp32 vector width: the kernels themselves are
    right at 9 vector columns, bias gradient included."""
    torch.manual_seed(0)
    x = torch.randn(33, 36, device="cuda")
    b = torch.randn(36, device="cuda")
    dy = torch.randn(33, 36, device="cuda")
    xr = x.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yr = torch.nn.functional.gelu(xr + br)
    yr.backward(dy)
    y = _ext().bias_gelu_fwd(x, b)
    dx, db = _ext().bias_gelu_bwd(x, b, dy, True)
    assert _rel_err(y, yr) < 1e-5
    assert _rel_err(dx, xr.grad) < 3e-5 and _rel_err(db, br.grad) < 3e-5
    keep = elem_keep_mask(SEED_LO, 33 * 36, 0.5).view(33, 36).cuda().float()
    y2 = _ext().bias_dropout_res_fwd(x, b, dy, 0.5, SEED_LO)
    assert _rel_err(y2, dy + (x + b) * keep * 2.0) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,W", [(1000, 31), (3, 31), (1000, 512), (3, 8)])
def test_colsum_matches_fp32_sum(R, W, dtype):
    """Scalar (W=31) and vector kernels, one row group (R=3) and many."""
    torch.manual_seed(0)
    x = torch.randn(R, W, device="cuda", dtype=dtype)
    got = _ext().colsum(x, W)
    assert got.shape == (W,) and got.dtype == dtype
    want = x.double().sum(0)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    err = _rel_err(got.double(), want)
    _report("colsum", f"R{R} W{W} {dtype}", "rel", err, tol)
    assert err < tol
