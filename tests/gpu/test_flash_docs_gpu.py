"""Flash attention over packed documents (the DOCS kernels) vs an fp32 PyTorch
reference with an explicit block-diagonal causal mask: query i sees key j iff
doc_start[b, i] <= j <= i (and j < kv_len[b])."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# the project's bounds, as in tests/gpu/test_flash_window_gpu.py
FWD_TOL = 2e-2    # max-abs vs fp32
GRAD_TOL = 5e-2   # relative to the reference grad's max-abs

B, H = 2, 4
LAYOUT1 = [37, 1, 155, 63, 128]  # S = 384; see test 1
ALT_1_7 = [1, 7] * 16            # S = 128


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _bounds(rows, s):
    """rows: one list of document lengths per batch row -> (doc_start, doc_end),
    int32 [B, s] on the GPU."""
    from libai_amd.data.packing import doc_bounds_from_lengths

    per_row = [doc_bounds_from_lengths(r, s) for r in rows]
    ds = torch.stack([p[0] for p in per_row]).cuda().contiguous()
    de = torch.stack([p[1] for p in per_row]).cuda().contiguous()
    return ds, de


def _visible(doc_start, s, kv_len=None):
    """[B, 1, S, S] bool."""
    i = torch.arange(s, device="cuda")[:, None]
    j = torch.arange(s, device="cuda")[None, :]
    vis = (j <= i)[None] & (j[None] >= doc_start.long()[:, :, None])
    if kv_len is not None:
        vis = vis & (j[None] < kv_len.long()[:, None, None])
    return vis[:, None]


def _ref_docs(q, k, v, scale, doc_start, kv_len=None, keep=None):
    """fp32 reference on [B, S, H(q), D] / [B, S, Hkv, D] inputs.  Rows with no
    visible key give zeros, as the kernel does.  keep: optional [B, H, S, S]
    dropout factor (0 or 1 / (1 - p)) applied to the probabilities."""
    group = q.shape[2] // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    vh = v.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    visible = _visible(doc_start, s.shape[-1], kv_len)
    s = s.masked_fill(~visible, float("-inf"))
    has_key = visible.any(-1, keepdim=True)
    s = torch.where(has_key, s, torch.zeros_like(s))  # keep empty rows finite
    p = torch.softmax(s, dim=-1) * has_key
    if keep is not None:
        p = p * keep
    return torch.matmul(p, vh).permute(0, 2, 1, 3)


def _qkv(s, d, hkv=None, seed=0, grad=False, b=B):
    torch.manual_seed(seed)
    hkv = hkv or H
    mk = lambda n: torch.randn(b, s, n, d, device="cuda", dtype=torch.bfloat16,
                               requires_grad=grad)
    return mk(H), mk(hkv), mk(hkv)


def _zero_ref_bound(q, k, v, g, scale):
    """A row whose document has ONE visible key has P = 1, so the exact dS =
    P * (dO.V^T - rowsum(dO * O)) is 0; where that holds for every row the
    reference dQ and dK are identically zero and "relative to the reference's
    max-abs" has no scale.  The kernels form the two terms as separate fp32
    dot products of D bf16 products (the MFMA and the rowsum kernel sum in
    different orders), each within D * 2^-24 * sum|terms| <= D^2 * 2^-24 *
    max|dO| * max|V| of the exact value; dQ/dK multiply the difference by
    scale * K (or Q).  That worst case bounds the absolute error."""
    d = q.shape[-1]
    amax = lambda t: t.detach().float().abs().max().item()
    dot_err = d * d * 2.0 ** -24 * amax(g) * amax(v)
    return 2.0 * dot_err * scale * max(amax(q), amax(k))


def _check_grads(got_ref_pairs, tag, zero_ref_bound=None):
    for name, got, want in got_ref_pairs:
        assert torch.isfinite(got.float()).all(), f"{tag} {name} not finite"
        err = (got.float() - want).abs().max().item()
        if want.abs().max().item() == 0.0 and zero_ref_bound is not None:
            print(f"{tag} {name} abs err {err:.3e} (zero reference, bound "
                  f"{zero_ref_bound:.3e})")
            assert err < zero_ref_bound, f"{tag} {name} abs err {err}"
            continue
        rel = err / (want.abs().max().item() + 1e-6)
        print(f"{tag} {name} rel err {rel:.3e}")
        assert rel < GRAD_TOL, f"{tag} {name} rel err {rel}"


def _fwd_bwd_vs_ref(s, d, rows, hkv=None, kv_len=None, seed=0, tag=""):
    from libai_amd.ops.attention import flash_attention

    ds, de = _bounds(rows, s)
    q, k, v = _qkv(s, d, hkv=hkv, seed=seed, grad=True)
    scale = 1.0 / math.sqrt(d)
    o = flash_attention(q, k, v, scale, p_drop=0.0, causal=True, kv_len=kv_len,
                        doc_bounds=(ds, de))
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_docs(qr, kr, vr, scale, ds, kv_len=kv_len)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - ref).abs().max().item()
    print(f"{tag} s{s} d{d} fwd max err {err:.3e}")
    assert err < FWD_TOL, f"docs fwd max err {err}"

    g = torch.randn_like(ref)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = (torch.arange(s, device="cuda")[None, :] < kv_len[:, None]).float()
        g = g * qmask[:, :, None, None]
    o.backward(g.to(torch.bfloat16))
    ref.backward(g)
    _check_grads([("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                  ("dv", v.grad, vr.grad)], f"{tag} s{s} d{d}",
                 zero_ref_bound=_zero_ref_bound(q, k, v, g, scale))
    return q, k, v, o


# 1. forward + backward vs reference -------------------------------------------
# mixed:  boundaries inside sub-tiles, a one-token document, interior 64x32
#         forward sub-tiles inside the 155-token document, and a tile-aligned
#         boundary at 256 (round 0 and two bwd_kv q tiles are skipped); row 1 is
#         ONE document: every skip is off and the result is plain causal
# diag:   only the diagonal tiles are walked
# ragged: Sq no multiple of the block
# alt:    lengths alternating 1 and 7: many rows with a single key (P = 1)
_LAYOUTS = {
    "mixed": (384, [LAYOUT1, [384]]),
    "diag": (384, [[128, 128, 128]] * 2),
    "ragged": (200, [[8, 192], [200]]),
    "alt": (128, [ALT_1_7] * 2),
}


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_docs_fwd_bwd_matches_reference(d, name):
    s, rows = _LAYOUTS[name]
    _fwd_bwd_vs_ref(s, d, rows, tag=name)


# 2. GQA -----------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_docs_gqa_matches_reference(d):
    s, rows = _LAYOUTS["mixed"]
    _fwd_bwd_vs_ref(s, d, rows, hkv=1, seed=2, tag="gqa")


# 3. kv_len ----------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_docs_kv_len_padding_matches_reference(d):
    """Documents [50, 70] and 80 padding tokens (one-token documents)."""
    s = 200
    lens = torch.tensor([120, s], device="cuda", dtype=torch.int32)
    q, k, v, o = _fwd_bwd_vs_ref(s, d, [[50, 70], [50, 70]], kv_len=lens, seed=1,
                                 tag="kv_len")
    pad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert pad.any()
    assert k.grad.float()[pad].abs().max().item() == 0.0
    assert v.grad.float()[pad].abs().max().item() == 0.0
    # a padded query is its own one-token document and its only key is padded
    assert o.float()[pad].abs().max().item() == 0.0
    assert q.grad.float()[pad].abs().max().item() == 0.0


# 4. isolation, exact ---------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_docs_are_isolated_exactly(d):
    from libai_amd.ops._ext import ext

    s = 384
    ds, de = _bounds([LAYOUT1] * 2, s)
    q, k, v = _qkv(s, d, seed=5)
    scale = 1.0 / math.sqrt(d)
    lo, hi = 38, 38 + 155  # the 155-token document
    o1, lse1 = ext().flash_fwd(q, k, v, scale, 0.0, 0, True, None, None, 0, None,
                               ds, de)
    q2, k2, v2 = q.clone(), k.clone(), v.clone()
    torch.manual_seed(55)
    for t in (q2, k2, v2):
        t[:, lo:hi] = torch.randn_like(t[:, lo:hi])
    o2, lse2 = ext().flash_fwd(q2, k2, v2, scale, 0.0, 0, True, None, None, 0, None,
                               ds, de)
    other = torch.ones(s, dtype=torch.bool, device="cuda")
    other[lo:hi] = False
    assert torch.equal(o2[:, other], o1[:, other])
    assert torch.equal(lse2[:, :, other], lse1[:, :, other])
    assert not torch.equal(o2[:, lo:hi], o1[:, lo:hi])

    # upstream gradient on the 63-token document only
    glo, ghi = hi, hi + 63
    g = torch.zeros_like(o1)
    g[:, glo:ghi] = torch.randn_like(g[:, glo:ghi])
    dq, dk, dv = ext().flash_bwd(q, k, v, o1, g, lse1, scale, 0.0, 0, True, None,
                                 None, None, 0, None, ds, de)
    outside = torch.ones(s, dtype=torch.bool, device="cuda")
    outside[glo:ghi] = False
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t.float()).all()
        assert t.float()[:, outside].abs().max().item() == 0.0, name
        assert t.float()[:, glo:ghi].abs().max().item() > 0.0, name


# 5. per-document equivalence -----------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_docs_equal_each_document_alone(d):
    """Every document of the mixed layout alone through the plain causal
    kernels (padded to a multiple of 8 keys, kv_len = its length).  Both sides
    are bf16 kernels at different tile alignments: each is within the project's
    bounds of the exact result, measured on the scale of the document's fp32
    reference gradient; where that reference is identically zero (the
    one-token document's dQ and dK) both are within _zero_ref_bound of 0."""
    from libai_amd.ops.attention import flash_attention

    s = 384
    ds, de = _bounds([LAYOUT1] * 2, s)
    q, k, v = _qkv(s, d, seed=6, grad=True)
    scale = 1.0 / math.sqrt(d)
    torch.manual_seed(66)
    g = torch.randn(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    o = flash_attention(q, k, v, scale, causal=True, doc_bounds=(ds, de))
    o.backward(g)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    _ref_docs(qr, kr, vr, scale, ds).backward(g.float())
    zero_bound = _zero_ref_bound(q, k, v, g, scale)

    a = 0
    for n in LAYOUT1:
        n8 = (n + 7) // 8 * 8
        pad = lambda t: torch.nn.functional.pad(t.detach()[:, a:a + n],
                                                (0, 0, 0, 0, 0, n8 - n))
        qa, ka, va = (pad(t).requires_grad_(True) for t in (q, k, v))
        lens = torch.full((B,), n, device="cuda", dtype=torch.int32)
        oa = flash_attention(qa, ka, va, scale, causal=True, kv_len=lens)
        oa.backward(pad(g))
        err = (o[:, a:a + n].float() - oa[:, :n].float()).abs().max().item()
        print(f"d{d} doc@{a}+{n} fwd max diff {err:.3e}")
        assert err < FWD_TOL
        for name, got, alone, ref in (("dq", q.grad, qa.grad, qr.grad),
                                      ("dk", k.grad, ka.grad, kr.grad),
                                      ("dv", v.grad, va.grad, vr.grad)):
            diff = (got[:, a:a + n].float() - alone[:, :n].float()).abs().max().item()
            ref_max = ref[:, a:a + n].abs().max().item()
            bound = GRAD_TOL * ref_max if ref_max > 0 else 2 * zero_bound
            print(f"d{d} doc@{a}+{n} {name} max diff {diff:.3e} bound {bound:.3e}")
            assert diff < bound, f"doc@{a}+{n} {name}: {diff} >= {bound}"
        a += n


# 6. one document == the plain causal call ------------------------------------------------
@pytest.mark.parametrize("s", [200, 384])
@pytest.mark.parametrize("d", [64, 128])
def test_single_document_equals_plain_causal(d, s):
    from libai_amd.ops.attention import flash_attention

    ds, de = _bounds([[s]] * 2, s)
    scale = 1.0 / math.sqrt(d)
    torch.manual_seed(77)
    g = torch.randn(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    res = []
    for bounds in (None, (ds, de)):
        q, k, v = _qkv(s, d, seed=7, grad=True)
        o = flash_attention(q, k, v, scale, causal=True, doc_bounds=bounds)
        o.backward(g)
        res.append((o.detach(), q.grad, k.grad, v.grad))
    (o0, *g0), (o1, *g1) = res
    bit_equal = all(torch.equal(x, y) for x, y in zip(res[0], res[1]))
    print(f"d{d} s{s} one document vs plain causal: bit-equal = {bit_equal}")
    assert (o1.float() - o0.float()).abs().max().item() < FWD_TOL
    _check_grads([(n, x, y.float()) for n, x, y in zip(("dq", "dk", "dv"), g1, g0)],
                 f"d{d} s{s} one-doc")


# 7. dropout, same mask ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_docs_dropout_matches_same_mask_reference(d):
    """The dropout key stays (bh, q, kv4): attn_dropout_apply on a tensor of
    ones gives the factor the kernels apply, and the fp32 reference applies the
    same one.  Bounds as in tests/gpu/test_dropout_exact_gpu.py."""
    from libai_amd.ops._ext import ext

    s, p, seed = 384, 0.1, (1 << 61) + 0xDEADBEEF
    ds, de = _bounds([LAYOUT1, [384]], s)
    q, k, v = _qkv(s, d, seed=8)
    scale = 1.0 / math.sqrt(d)
    keep = torch.ones(B * H, s, s, device="cuda", dtype=torch.float32)
    ext().attn_dropout_apply(keep, s, s, p, seed)
    keep = keep.view(B, H, s, s)
    assert 0.85 < (keep != 0).float().mean().item() < 0.95

    o, lse = ext().flash_fwd(q, k, v, scale, p, seed, True, None, None, 0, None,
                             ds, de)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_docs(qr, kr, vr, scale, ds, keep=keep)
    assert torch.isfinite(o.float()).all()
    err = (o.float() - ref).abs().max().item()
    print(f"dropout d{d} fwd max err {err:.3e} bound {FWD_TOL / (1 - p):.3e}")
    assert err < FWD_TOL / (1 - p)
    torch.manual_seed(88)
    g = torch.randn(B, s, H, d, device="cuda").to(torch.bfloat16)
    dq, dk, dv = ext().flash_bwd(q, k, v, o, g, lse, scale, p, seed, True, None,
                                 None, None, 0, None, ds, de)
    ref.backward(g.float())
    _check_grads([("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)],
                 f"dropout d{d}")


# 8. packed qkv path ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_docs_packed_qkv_equals_view_path(d):
    from libai_amd.ops.attention import flash_attention, flash_attention_qkv

    s = 384
    ds, de = _bounds([LAYOUT1, [384]], s)
    torch.manual_seed(9)
    qkv = torch.randn(B, s, H, 3, d, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(B, s, H, d, device="cuda", dtype=torch.bfloat16)
    scale = d ** -0.5
    a = qkv.clone().requires_grad_(True)
    o_packed = flash_attention_qkv(a, scale, causal=True, doc_bounds=(ds, de))
    o_packed.backward(g)
    b = qkv.clone().requires_grad_(True)
    o_views = flash_attention(b[..., 0, :], b[..., 1, :], b[..., 2, :], scale,
                              causal=True, doc_bounds=(ds, de))
    o_views.backward(g)
    assert torch.equal(o_packed, o_views)
    assert torch.equal(a.grad, b.grad)
    # and the documents really are applied on this path
    with torch.no_grad():
        o_plain = flash_attention_qkv(qkv, scale, causal=True)
    assert not torch.equal(o_plain[0], o_packed[0])


# 9. rejections -----------------------------------------------------------------------------------
def test_doc_bounds_rejections():
    from libai_amd.ops._ext import ext
    from libai_amd.ops.attention import flash_attention, flash_attention_qkv

    s = 128
    q, k, v = _qkv(s, 64, seed=10)
    ds, de = _bounds([[40, 88]] * 2, s)
    slopes = torch.ones(H, device="cuda", dtype=torch.float32)
    table = torch.zeros(H, 2 * s - 1, device="cuda", dtype=torch.float32)
    for kw in (dict(alibi_slopes=slopes), dict(window=16), dict(rel_bias=table),
               dict(causal=False)):
        with pytest.raises(ValueError):
            flash_attention(q, k, v, 0.125, doc_bounds=(ds, de), **kw)
    qkv = torch.stack([q, k, v], dim=3)
    with pytest.raises(ValueError):
        flash_attention_qkv(qkv, 0.125, causal=False, doc_bounds=(ds, de))
    with pytest.raises(ValueError):
        flash_attention(q, k, v, 0.125, doc_bounds=(ds, None))

    # the binding itself: fwd(q, k, v, scale, p, seed, causal, kv_len, slopes,
    # window, rel_bias, doc_start, doc_end)
    fwd = lambda *a: ext().flash_fwd(q, k, v, 0.125, 0.0, 0, *a)
    with pytest.raises(RuntimeError, match="alibi"):
        fwd(True, None, slopes, 0, None, ds, de)
    with pytest.raises(RuntimeError, match="window"):
        fwd(True, None, None, 16, None, ds, de)
    with pytest.raises(RuntimeError, match="rel_bias"):
        fwd(True, None, None, 0, table, ds, de)
    with pytest.raises(RuntimeError, match="causal"):
        fwd(False, None, None, 0, None, ds, de)
    with pytest.raises(RuntimeError, match="int32"):       # wrong dtype
        fwd(True, None, None, 0, None, ds.long(), de.long())
    with pytest.raises(RuntimeError, match="shape"):       # wrong shape
        fwd(True, None, None, 0, None, ds[:, :64].contiguous(),
            de[:, :64].contiguous())
    with pytest.raises(RuntimeError, match="shape"):
        fwd(True, None, None, 0, None, ds[0].contiguous(), de[0].contiguous())
    with pytest.raises(RuntimeError, match="together"):    # not both
        fwd(True, None, None, 0, None, ds, None)
    with pytest.raises(RuntimeError, match="together"):
        fwd(True, None, None, 0, None, None, de)
    o, lse = fwd(True, None, None, 0, None, ds, de)
    with pytest.raises(RuntimeError, match="together"):
        ext().flash_bwd(q, k, v, o, torch.ones_like(o), lse, 0.125, 0.0, 0, True,
                        None, None, None, 0, None, ds, None)
    with pytest.raises(RuntimeError, match="int32"):
        ext().flash_bwd(q, k, v, o, torch.ones_like(o), lse, 0.125, 0.0, 0, True,
                        None, None, None, 0, None, ds.long(), de.long())
