"""Fused ALiBi in the flash-attention and decode kernels vs an fp32 PyTorch
reference whose bias is built in fp32 as slope[h] * (j - i)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2    # max-abs, fwd and decode (the project's bound vs fp32)
GRAD_TOL = 5e-2   # relative to the reference grad's max-abs


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _slopes(h):
    from libai_amd.layers.position_bias import alibi_slopes

    return alibi_slopes(h).to(device="cuda", dtype=torch.float32).contiguous()


def _ref_alibi(q, k, v, scale, causal, slopes, kv_len=None, form="rel"):
    """fp32 reference on [B, S, H(q), D] / [B, S, Hkv, D] inputs."""
    group = q.shape[2] // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    vh = v.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    sq, sk = s.shape[-2], s.shape[-1]
    i = torch.arange(sq, device=q.device, dtype=torch.float32)[:, None]
    j = torch.arange(sk, device=q.device, dtype=torch.float32)[None, :]
    rel = (j - i) if form == "rel" else j.expand(sq, sk)
    s = s + slopes.float()[None, :, None, None] * rel[None, None]
    if kv_len is not None:
        pad = (torch.arange(sk, device=q.device)[None, None, None, :]
               >= kv_len[:, None, None, None])
        s = s.masked_fill(pad, float("-inf"))
    if causal:
        cm = torch.ones(sq, sk, dtype=torch.bool, device=q.device).tril_(sk - sq)
        s = s.masked_fill(~cm, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, vh).permute(0, 2, 1, 3)


def _qkv(b, s, h, d, hkv=None, seed=0, grad=False):
    torch.manual_seed(seed)
    hkv = hkv or h
    mk = lambda n: torch.randn(b, s, n, d, device="cuda", dtype=torch.bfloat16,
                               requires_grad=grad)
    return mk(h), mk(hkv), mk(hkv)


def _check_grads(got_ref_pairs, tag):
    for name, got, want in got_ref_pairs:
        rel = ((got.float() - want).abs().max() / (want.abs().max() + 1e-6)).item()
        print(f"{tag} {name} rel err {rel:.3e}")
        assert rel < GRAD_TOL, f"{tag} {name} rel err {rel}"


def _fwd_bwd_vs_ref(b, s, h, d, causal, hkv=None, kv_len=None, seed=0):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(b, s, h, d, hkv=hkv, seed=seed, grad=True)
    slopes = _slopes(h)
    scale = 1.0 / math.sqrt(d)
    o = flash_attention(q, k, v, scale, p_drop=0.0, causal=causal, kv_len=kv_len,
                        alibi_slopes=slopes)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_alibi(qr, kr, vr, scale, causal, slopes, kv_len=kv_len)
    err = (o.float() - ref).abs().max().item()
    print(f"fwd max err {err:.3e}")
    assert err < FWD_TOL, f"alibi fwd max err {err}"

    g = torch.randn_like(ref)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = (torch.arange(s, device="cuda")[None, :] < kv_len[:, None]).float()
        g = g * qmask[:, :, None, None]
    o.backward(g.to(torch.bfloat16))
    ref.backward(g)
    _check_grads([("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                  ("dv", v.grad, vr.grad)], f"s{s} d{d}")
    return q, k, v


# 1. forward -----------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("s", [128, 200, 384])
def test_alibi_fwd_matches_reference(d, causal, s):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(2, s, 4, d)
    slopes = _slopes(4)
    scale = 1.0 / math.sqrt(d)
    o = flash_attention(q, k, v, scale, p_drop=0.0, causal=causal,
                        alibi_slopes=slopes)
    ref = _ref_alibi(q, k, v, scale, causal, slopes)
    err = (o.float() - ref).abs().max().item()
    print(f"fwd max err {err:.3e}")
    assert err < FWD_TOL, f"alibi fwd max err {err}"
    # slope*(j - i) and BLOOM's slope*j are the same attention
    ref_j = _ref_alibi(q, k, v, scale, causal, slopes, form="abs")
    assert (ref - ref_j).abs().max().item() < 1e-4


# 2. forward + backward --------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("s", [200, 384])
def test_alibi_backward_matches_reference_causal(d, s):
    _fwd_bwd_vs_ref(2, s, 4, d, causal=True)


def test_alibi_backward_matches_reference_noncausal():
    _fwd_bwd_vs_ref(2, 200, 4, 64, causal=False)


# 3. GQA: the slope belongs to the QUERY head ----------------------------------
@pytest.mark.parametrize("group", [2, 4])
def test_alibi_gqa_matches_reference(group):
    _fwd_bwd_vs_ref(2, 256, 8, 64, causal=True, hkv=8 // group, seed=2)


# 4. kv_len + ALiBi --------------------------------------------------------------
def test_alibi_kv_len_padding_matches_reference():
    lens = torch.tensor([200, 136, 57, 1], device="cuda", dtype=torch.int32)
    s = 200
    _, k, v = _fwd_bwd_vs_ref(4, s, 4, 64, causal=True, kv_len=lens, seed=1)
    kpad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert k.grad.float()[kpad].abs().max().item() == 0.0
    assert v.grad.float()[kpad].abs().max().item() == 0.0


# 5. packed qkv path ---------------------------------------------------------------
def test_alibi_qkv_packed_matches_view_path():
    from libai_amd.ops.attention import flash_attention, flash_attention_qkv

    torch.manual_seed(7)
    b, s, h, d = 2, 256, 4, 64
    slopes = _slopes(h)
    qkv = torch.randn(b, s, h, 3, d, device="cuda", dtype=torch.bfloat16)
    q1 = qkv.clone().requires_grad_(True)
    q2 = qkv.clone().requires_grad_(True)
    o1 = flash_attention_qkv(q1, scale=d ** -0.5, p_drop=0.0, causal=True,
                             alibi_slopes=slopes)
    o2 = flash_attention(q2[..., 0, :], q2[..., 1, :], q2[..., 2, :],
                         scale=d ** -0.5, p_drop=0.0, causal=True,
                         alibi_slopes=slopes)
    assert torch.equal(o1, o2)
    g = torch.randn_like(o1)
    o1.backward(g)
    o2.backward(g)
    assert torch.equal(q1.grad, q2.grad)


# 6. dropout + ALiBi -----------------------------------------------------------------
def test_alibi_dropout_backward_finite_and_eval_is_exact():
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(2, 128, 2, 64, grad=True)
    slopes = _slopes(2)
    o = flash_attention(q, k, v, 0.125, p_drop=0.1, causal=True,
                        alibi_slopes=slopes)
    o.sum().backward()
    for t in (o, q.grad, k.grad, v.grad):
        assert torch.isfinite(t.float()).all()
    with torch.no_grad():
        o_eval = flash_attention(q, k, v, 0.125, p_drop=0.1, causal=True,
                                 training=False, alibi_slopes=slopes)
        o_p0 = flash_attention(q, k, v, 0.125, p_drop=0.0, causal=True,
                               alibi_slopes=slopes)
    assert torch.equal(o_eval, o_p0)


# 7. the slopes are actually used ------------------------------------------------------
def test_alibi_slopes_change_output_and_zero_slopes_do_not():
    from libai_amd.ops.attention import flash_attention

    for d in (64, 128):
        q, k, v = _qkv(2, 384, 4, d)
        scale = 1.0 / math.sqrt(d)
        o_none = flash_attention(q, k, v, scale, causal=True)
        o_alibi = flash_attention(q, k, v, scale, causal=True,
                                  alibi_slopes=_slopes(4))
        diff = (o_alibi.float() - o_none.float()).abs().max().item()
        assert diff > FWD_TOL, f"slopes ignored? max diff {diff}"
        zeros = torch.zeros(4, device="cuda", dtype=torch.float32)
        o_zero = flash_attention(q, k, v, scale, causal=True, alibi_slopes=zeros)
        assert torch.equal(o_zero, o_none)


# 8. decode ----------------------------------------------------------------------------
def _ref_decode(q, k, v, scale, slopes, lens):
    """q [B,H,1,D], k/v [B,Hkv,S,D]; the query sits at key index lens[b]-1."""
    group = q.shape[1] // k.shape[1]
    skv = k.shape[2]
    kx = k.float().repeat_interleave(group, dim=1)
    vx = v.float().repeat_interleave(group, dim=1)
    s = torch.matmul(q.float(), kx.transpose(-1, -2)) * scale  # [B,H,1,S]
    j = torch.arange(skv, device=q.device, dtype=torch.float32)
    rel = j[None, :] - (lens.float()[:, None] - 1.0)            # [B,S]
    s = s + slopes.float()[None, :, None, None] * rel[:, None, None, :]
    mask = torch.arange(skv, device=q.device)[None, :] >= lens[:, None]
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vx)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("group", [1, 4])
def test_alibi_decode_matches_reference(d, group):
    from libai_amd.ops.attention import flash_decode_attn

    torch.manual_seed(3)
    b, hq, skv = 3, 8, 229
    hkv = hq // group
    q = torch.randn(b, hq, 1, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, hkv, skv, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(b, hkv, skv, d, device="cuda", dtype=torch.bfloat16)
    slopes = _slopes(hq)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_decode_attn(q, k, v, scale, alibi_slopes=slopes)
        full = torch.full((b,), skv, device="cuda", dtype=torch.int32)
        ref = _ref_decode(q, k, v, scale, slopes, full)
        err = (o.float() - ref).abs().max().item()
        assert err < FWD_TOL, f"alibi decode max err {err}"

        lens = torch.tensor([229, 100, 1], device="cuda", dtype=torch.int32)
        o2 = flash_decode_attn(q, k, v, scale, kv_len=lens, alibi_slopes=slopes)
        ref2 = _ref_decode(q, k, v, scale, slopes, lens)
        err2 = (o2.float() - ref2).abs().max().item()
        assert err2 < FWD_TOL, f"alibi decode kv_len max err {err2}"
        # and the bias is really applied
        o_none = flash_decode_attn(q, k, v, scale)
        assert (o.float() - o_none.float()).abs().max().item() > FWD_TOL


def test_alibi_decode_split_kv_capacity_independent():
    from libai_amd.ops.attention import flash_decode_attn

    torch.manual_seed(0)
    B, H, D, L = 4, 16, 64, 450
    slopes = _slopes(H)
    q = torch.randn(B, H, 1, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, H, L, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn_like(k)
    kvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    scale = D ** -0.5

    def with_capacity(cap):
        kc = torch.randn(B, H, cap, D, device="cuda", dtype=torch.bfloat16)
        vc = torch.randn_like(kc)
        kc[:, :, :L].copy_(k)
        vc[:, :, :L].copy_(v)
        return flash_decode_attn(q, kc, vc, scale, kv_len=kvl, alibi_slopes=slopes)

    with torch.no_grad():
        o_small = with_capacity(512)    # single-WG kernel
        o_big = with_capacity(1536)     # split path, 2 null splits
        assert torch.equal(o_small, o_big)
        ref = _ref_decode(q, k, v, scale, slopes, kvl)
        assert (o_big.float() - ref).abs().max().item() < FWD_TOL

        # several REAL splits, per-batch lengths
        B2, cap2 = 2, 1536
        q2 = torch.randn(B2, H, 1, D, device="cuda", dtype=torch.bfloat16)
        k2 = torch.randn(B2, H, cap2, D, device="cuda", dtype=torch.bfloat16)
        v2 = torch.randn_like(k2)
        kvl2 = torch.tensor([1300, 700], dtype=torch.int32, device="cuda")
        o2 = flash_decode_attn(q2, k2, v2, scale, kv_len=kvl2, alibi_slopes=slopes)
        ref2 = _ref_decode(q2, k2, v2, scale, slopes, kvl2)
        err = (o2.float() - ref2).abs().max().item()
        assert err < FWD_TOL, f"alibi split decode max err {err}"


# 9. layer and model routing ---------------------------------------------------------
def _record(monkeypatch, name):
    """Wrap ops.attention.<name>, recording the alibi_slopes of each call."""
    import libai_amd.ops.attention as A

    calls = []
    orig = getattr(A, name)

    def wrapper(*a, **kw):
        calls.append(kw.get("alibi_slopes"))
        return orig(*a, **kw)

    monkeypatch.setattr(A, name, wrapper)
    return calls


def test_layer_alibi_bias_takes_flash_route(monkeypatch):
    from libai_amd import layers
    from libai_amd.layers.position_bias import build_alibi_bias

    torch.manual_seed(0)
    attn = layers.MultiheadAttention(256, 4, attn_mask_type="causal")
    attn = attn.to(torch.bfloat16).cuda().eval()
    x = torch.randn(2, 128, 256, device="cuda", dtype=torch.bfloat16)
    bias = build_alibi_bias(4, 128, device="cuda", dtype=torch.bfloat16)
    calls = _record(monkeypatch, "flash_attention_qkv")
    with torch.no_grad():
        y_flash = attn(x, position_bias=bias)
        assert len(calls) == 1 and calls[0] is not None
        assert calls[0].dtype == torch.float32 and calls[0].numel() == 4
        # a cache request forces the materialized-bias route
        y_unfused, _ = attn(x, position_bias=bias, use_cache=True)
        assert len(calls) == 1
    rel = ((y_flash.float() - y_unfused.float()).abs().max()
           / (y_unfused.float().abs().max() + 1e-6)).item()
    assert rel < 3e-2, f"alibi flash vs unfused layer mismatch {rel}"
    # the bias must matter at this shape, or the comparison shows nothing
    with torch.no_grad():
        y_nobias = attn(x)
    assert (y_flash.float() - y_nobias.float()).abs().max().item() > 0


def test_layer_plain_bias_keeps_materialized_route(monkeypatch):
    from libai_amd import layers

    torch.manual_seed(0)
    attn = layers.MultiheadAttention(256, 4, attn_mask_type="causal")
    attn = attn.to(torch.bfloat16).cuda().eval()
    x = torch.randn(2, 128, 256, device="cuda", dtype=torch.bfloat16)
    bias = torch.randn(4, 128, 128, device="cuda", dtype=torch.bfloat16)
    calls = _record(monkeypatch, "flash_attention_qkv")
    with torch.no_grad():
        y = attn(x, position_bias=bias)
        y_cache, _ = attn(x, position_bias=bias, use_cache=True)
    assert calls == []
    assert torch.equal(y, y_cache)


def test_bloom_decode_uses_fused_alibi_and_matches_full(monkeypatch):
    from libai_amd.models import BloomForCausalLM

    torch.manual_seed(0)
    m = BloomForCausalLM(vocab_size=512, hidden_size=256, hidden_layers=2,
                         num_attention_heads=4).to(torch.bfloat16).cuda().eval()
    ids = torch.randint(0, 512, (2, 40), device="cuda")
    fwd_calls = _record(monkeypatch, "flash_attention_qkv")
    dec_calls = _record(monkeypatch, "flash_decode_attn")
    with torch.no_grad():
        full = m(input_ids=ids)["prediction_scores"]
        assert len(fwd_calls) == 2 and all(c is not None for c in fwd_calls)
        o = m(input_ids=ids[:, :32], use_cache=True)
        st = m(input_ids=ids[:, 32:33], past_key_values=o["past_key_values"],
               use_cache=True)
    assert len(dec_calls) == 2 and all(c is not None for c in dec_calls)
    err = (st["prediction_scores"][:, 0].float() - full[:, 32].float()).abs().max()
    assert err.item() < 0.1, err.item()
