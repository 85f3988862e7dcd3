"""Sliding-window (Mistral) attention in the flash and decode kernels vs an
fp32 PyTorch reference with an explicit band mask: query i sees key j iff
j <= i and i - j < W (and j < kv_len[b])."""

import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2    # max-abs, fwd and decode (the project's bound vs fp32)
GRAD_TOL = 5e-2   # relative to the reference grad's max-abs
LAYER_TOL = 3e-2  # flash vs unfused layer output, relative
LOGIT_TOL = 0.1   # decode step vs full forward, model logits


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _ref_window(q, k, v, scale, window, kv_len=None):
    """fp32 reference on [B, S, H(q), D] / [B, S, Hkv, D] inputs.  Rows with
    no visible key (padded query rows) give zeros, as the kernel does."""
    group = q.shape[2] // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    vh = v.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    sq, sk = s.shape[-2], s.shape[-1]
    i = torch.arange(sq, device=q.device)[:, None]
    j = torch.arange(sk, device=q.device)[None, :]
    visible = ((j <= i) & (i - j < window))[None, None]
    if kv_len is not None:
        visible = visible & (j[None, None] < kv_len[:, None, None, None])
    s = s.masked_fill(~visible, float("-inf"))
    has_key = visible.any(-1, keepdim=True)
    s = torch.where(has_key, s, torch.zeros_like(s))  # keep empty rows finite
    p = torch.softmax(s, dim=-1) * has_key
    return torch.matmul(p, vh).permute(0, 2, 1, 3)


def _qkv(b, s, h, d, hkv=None, seed=0, grad=False):
    torch.manual_seed(seed)
    hkv = hkv or h
    mk = lambda n: torch.randn(b, s, n, d, device="cuda", dtype=torch.bfloat16,
                               requires_grad=grad)
    return mk(h), mk(hkv), mk(hkv)


def _check_grads(got_ref_pairs, tag, zero_ref_bound=None):
    for name, got, want in got_ref_pairs:
        assert torch.isfinite(got.float()).all(), f"{tag} {name} not finite"
        err = (got.float() - want).abs().max().item()
        if want.abs().max().item() == 0.0 and zero_ref_bound is not None:
            # no scale to be relative to: see _zero_ref_bound
            print(f"{tag} {name} abs err {err:.3e} (zero reference, bound "
                  f"{zero_ref_bound:.3e})")
            assert err < zero_ref_bound, f"{tag} {name} abs err {err}"
            continue
        rel = err / (want.abs().max().item() + 1e-6)
        print(f"{tag} {name} rel err {rel:.3e}")
        assert rel < GRAD_TOL, f"{tag} {name} rel err {rel}"


def _zero_ref_bound(q, k, v, g, scale):
    """With W=1 every row's softmax is over ONE key: P = 1, so the exact dS =
    P * (dO.V^T - rowsum(dO * O)) is 0 and the reference dQ and dK are
    identically zero: "relative to the reference's max-abs" has no scale.
    The kernels form the two terms as separate fp32 dot products of D bf16
    products (the MFMA and the rowsum kernel sum in different orders), each
    within D * 2^-24 * sum|terms| <= D^2 * 2^-24 * max|dO| * max|V| of the
    exact value; dQ/dK multiply the difference by scale * K (or Q).  That
    worst case bounds the absolute error."""
    d = q.shape[-1]
    amax = lambda t: t.detach().float().abs().max().item()
    dot_err = d * d * 2.0 ** -24 * amax(g) * amax(v)
    return 2.0 * dot_err * scale * max(amax(q), amax(k))


def _fwd_bwd_vs_ref(b, s, h, d, window, hkv=None, kv_len=None, seed=0):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(b, s, h, d, hkv=hkv, seed=seed, grad=True)
    scale = 1.0 / math.sqrt(d)
    o = flash_attention(q, k, v, scale, p_drop=0.0, causal=True, kv_len=kv_len,
                        window=window)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = _ref_window(qr, kr, vr, scale, window, kv_len=kv_len)
    err = (o.float() - ref).abs().max().item()
    print(f"s{s} d{d} w{window} fwd max err {err:.3e}")
    assert err < FWD_TOL, f"window fwd max err {err}"

    g = torch.randn_like(ref)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = (torch.arange(s, device="cuda")[None, :] < kv_len[:, None]).float()
        g = g * qmask[:, :, None, None]
    o.backward(g.to(torch.bfloat16))
    ref.backward(g)
    _check_grads([("dq", q.grad, qr.grad), ("dk", k.grad, kr.grad),
                  ("dv", v.grad, vr.grad)], f"s{s} d{d} w{window}",
                 zero_ref_bound=_zero_ref_bound(q, k, v, g, scale))
    return q, k, v, o


# 1. forward + backward vs reference -------------------------------------------
# S: one q block / a ragged tail / three q blocks (the round-start skip and the
# bwd_kv q-tile cut both engage).  W >= S is "off"; one such case is kept.
_CASES = [(s, w) for s in (128, 200, 384) for w in (1, 2, 63, 64, 65, 129, 200)
          if w < s] + [(128, 129)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("s,window", _CASES)
def test_window_fwd_bwd_matches_reference(d, s, window):
    _fwd_bwd_vs_ref(2, s, 4, d, window)


@pytest.mark.parametrize("d", [64, 128])
def test_window_gqa_matches_reference(d):
    _fwd_bwd_vs_ref(2, 384, 4, d, 65, hkv=1, seed=2)


# short = 40: the query rows i >= 40 + 63 see no key at all
@pytest.mark.parametrize("short", [200 - 37, 40])
@pytest.mark.parametrize("d", [64, 128])
def test_window_kv_len_padding_matches_reference(d, short):
    s, w = 200, 64
    lens = torch.tensor([s, short], device="cuda", dtype=torch.int32)
    q, k, v, o = _fwd_bwd_vs_ref(2, s, 4, d, w, kv_len=lens, seed=1)
    pad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert k.grad.float()[pad].abs().max().item() == 0.0
    assert v.grad.float()[pad].abs().max().item() == 0.0
    # a query row with no visible key: exact zeros out and a zero dQ row
    empty = torch.arange(s, device="cuda")[None, :] >= lens[:, None] + (w - 1)
    if empty.any():
        assert o.float()[empty].abs().max().item() == 0.0
        assert q.grad.float()[empty].abs().max().item() == 0.0


# 2. keys outside the window have no influence -----------------------------------
def test_window_outside_keys_have_no_influence():
    """K/V rows j < 256 overwritten with 1.0e4 (finite on purpose: 0 * NaN
    would poison the MFMA).  With W=64 the rows i >= 320 see only j >= 257, so
    the same kernel must give bitwise the same rows, and a loss on those rows
    leaves dK/dV of the overwritten keys exactly zero."""
    from libai_amd.ops.attention import flash_attention

    s, w, d, cut, first = 512, 64, 64, 256, 320
    q, k, v = _qkv(2, s, 4, d, seed=5)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o_clean = flash_attention(q, k, v, scale, causal=True, window=w)
        kp, vp = k.clone(), v.clone()
        kp[:, :cut] = 1.0e4
        vp[:, :cut] = 1.0e4
        o_poison = flash_attention(q, kp, vp, scale, causal=True, window=w)
    assert torch.equal(o_poison[:, first:], o_clean[:, first:])
    # and the rows that do see the overwritten keys changed
    assert not torch.equal(o_poison[:, :cut], o_clean[:, :cut])

    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, kp, vp))
    o = flash_attention(qg, kg, vg, scale, causal=True, window=w)
    g = torch.randn_like(o)
    g[:, :first] = 0
    o.backward(g)
    assert kg.grad[:, :cut].float().abs().max().item() == 0.0
    assert vg.grad[:, :cut].float().abs().max().item() == 0.0
    assert kg.grad[:, first:].float().abs().max().item() > 0.0
    for t in (qg.grad, kg.grad, vg.grad):
        assert torch.isfinite(t.float()).all()


# 3. full-length window == no window ------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_full_length_window_equals_no_window(d):
    from libai_amd.ops._ext import ext
    from libai_amd.ops.attention import flash_attention

    s = 384
    q, k, v = _qkv(2, s, 4, d, seed=3)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o_none = flash_attention(q, k, v, scale, causal=True)
        o_full = flash_attention(q, k, v, scale, causal=True, window=s)
        # the windowed instantiation itself at W = S (no Python normalization)
        o_kern, _ = ext().flash_fwd(q, k, v, scale, 0.0, 0, True, None, None, s)
    assert (o_full.float() - o_none.float()).abs().max().item() < FWD_TOL
    assert (o_kern.float() - o_none.float()).abs().max().item() < FWD_TOL


def test_binding_rejects_window_with_alibi_or_noncausal():
    from libai_amd.ops._ext import ext

    q, k, v = _qkv(1, 128, 2, 64)
    slopes = torch.ones(2, device="cuda", dtype=torch.float32)
    with pytest.raises(RuntimeError, match="alibi"):
        ext().flash_fwd(q, k, v, 0.125, 0.0, 0, True, None, slopes, 16)
    with pytest.raises(RuntimeError, match="causal"):
        ext().flash_fwd(q, k, v, 0.125, 0.0, 0, False, None, None, 16)
    qd = q[:, :1].permute(0, 2, 1, 3).contiguous()
    kd = k.permute(0, 2, 1, 3)
    with pytest.raises(RuntimeError, match="alibi"):
        ext().flash_decode(qd, kd, kd, 0.125, None, slopes, 16)


# 4. dropout -----------------------------------------------------------------------
def test_window_dropout_finite_and_mean_preserved():
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(2, 384, 4, 64, seed=4, grad=True)
    o = flash_attention(q, k, v, 0.125, p_drop=0.1, causal=True, window=64)
    o.sum().backward()
    for t in (o, q.grad, k.grad, v.grad):
        assert torch.isfinite(t.float()).all()
    # V = ones: each output element = sum of kept P / (1 - p); mean ~ 1
    with torch.no_grad():
        ones = torch.ones_like(v)
        o1 = flash_attention(q, k, ones, 0.125, p_drop=0.1, causal=True, window=64)
        mean = o1.float().mean().item()
        assert abs(mean - 1.0) < 0.05, f"dropout-scaled mean {mean} != 1"
        o_eval = flash_attention(q, k, ones, 0.125, p_drop=0.1, causal=True,
                                 training=False, window=64)
        assert (o_eval.float() - 1.0).abs().max().item() < 0.05


# 5-7. decode ------------------------------------------------------------------------
def _ref_decode(q, k, v, scale, window, lens):
    """q [B,H,1,D], k/v [B,Hkv,S,D]; the query sits at key index lens[b]-1 and
    sees the keys [max(0, lens[b] - W), lens[b])."""
    group = q.shape[1] // k.shape[1]
    skv = k.shape[2]
    kx = k.float().repeat_interleave(group, dim=1)
    vx = v.float().repeat_interleave(group, dim=1)
    s = torch.matmul(q.float(), kx.transpose(-1, -2)) * scale  # [B,H,1,S]
    j = torch.arange(skv, device=q.device)[None, :]
    mask = (j >= lens[:, None]) | (j < lens[:, None] - window)
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vx)


@pytest.mark.parametrize("window", [1, 64, 100, 300])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("group", [1, 4])
def test_window_decode_matches_reference(group, d, window):
    from libai_amd.ops.attention import flash_decode_attn

    torch.manual_seed(3)
    b, hq, skv = 3, 8, 229
    hkv = hq // group
    q = torch.randn(b, hq, 1, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(b, hkv, skv, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(b, hkv, skv, d, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        full = torch.full((b,), skv, device="cuda", dtype=torch.int32)
        o = flash_decode_attn(q, k, v, scale, window=window)
        err = (o.float() - _ref_decode(q, k, v, scale, window, full)).abs().max().item()
        assert err < FWD_TOL, f"window decode max err {err}"

        lens = torch.tensor([229, 100, 1], device="cuda", dtype=torch.int32)
        o2 = flash_decode_attn(q, k, v, scale, kv_len=lens, window=window)
        ref2 = _ref_decode(q, k, v, scale, window, lens)
        err2 = (o2.float() - ref2).abs().max().item()
        assert err2 < FWD_TOL, f"window decode kv_len max err {err2}"
        if window < 100:  # the window is really applied
            o_none = flash_decode_attn(q, k, v, scale, kv_len=lens)
            assert (o2.float() - o_none.float()).abs().max().item() > FWD_TOL


# window start inside a split / exactly on a 512 boundary / one past it /
# before key 0 (for kv_len 1300 and 700)
@pytest.mark.parametrize("window", [1, 200, 512, 513, 788, 2000])
def test_window_decode_split_path_matches_reference(window):
    from libai_amd.ops.attention import flash_decode_attn

    torch.manual_seed(0)
    B, H, D, cap = 2, 16, 64, 1536
    q = torch.randn(B, H, 1, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, H, cap, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn_like(k)
    lens = torch.tensor([1300, 700], dtype=torch.int32, device="cuda")
    scale = D ** -0.5
    with torch.no_grad():
        o = flash_decode_attn(q, k, v, scale, kv_len=lens, window=window)
        ref = _ref_decode(q, k, v, scale, window, lens)
    err = (o.float() - ref).abs().max().item()
    assert err < FWD_TOL, f"window split decode max err {err}"


def test_window_decode_capacity_independent():
    from libai_amd.ops.attention import flash_decode_attn

    torch.manual_seed(0)
    B, H, D, L, W = 4, 16, 64, 450, 100
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
        return flash_decode_attn(q, kc, vc, scale, kv_len=kvl, window=W)

    with torch.no_grad():
        o_small = with_capacity(512)    # single-WG kernel
        o_big = with_capacity(1536)     # split path, 2 null splits
        assert torch.equal(o_small, o_big)
        ref = _ref_decode(q, k, v, scale, W, kvl)
        assert (o_big.float() - ref).abs().max().item() < FWD_TOL


# 8. decode agrees with the training kernel ---------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_window_decode_agrees_with_training_kernel(d):
    from libai_amd.ops.attention import flash_attention, flash_decode_attn

    s, w = 256, 80
    q, k, v = _qkv(2, s, 8, d, hkv=2, seed=6)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, window=w)
        qd = q[:, -1:].permute(0, 2, 1, 3).contiguous()           # [B,H,1,D]
        od = flash_decode_attn(qd, k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3),
                               scale, window=w)
    err = (od[:, :, 0].float() - o[:, -1].float()).abs().max().item()
    assert err < FWD_TOL, f"decode vs training kernel last row {err}"


# 9. model level -----------------------------------------------------------------------
def _tiny_windowed_llama(window=16):
    from libai_amd.models.llama import LlamaForCausalLM

    torch.manual_seed(1)
    m = LlamaForCausalLM(
        hidden_layers=4, vocab_size=1024, hidden_size=256,
        intermediate_size=512, num_attention_heads=4,
        num_key_value_heads=2, max_position_embeddings=1024,
        sliding_window=window,
    )
    return m.to("cuda", torch.bfloat16).eval()


def _record_ext(monkeypatch, name, window_pos):
    """Wrap the extension op, recording the window argument of each call."""
    from libai_amd.ops._ext import ext

    calls = []
    orig = getattr(ext(), name)

    def wrapper(*a, **kw):
        calls.append(kw.get("window", a[window_pos] if len(a) > window_pos else 0))
        return orig(*a, **kw)

    monkeypatch.setattr(ext(), name, wrapper)
    return calls


def test_model_training_forward_uses_windowed_flash(monkeypatch):
    import libai_amd.models.llama as L

    model = _tiny_windowed_llama()
    ids = torch.randint(0, 1024, (2, 128), device="cuda")
    calls = _record_ext(monkeypatch, "flash_fwd", 9)
    with torch.no_grad():
        model(input_ids=ids)
    assert calls == [16] * 4, calls

    attn = model.model.layers[0].self_attn
    x = torch.randn(2, 128, 256, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        y_flash = attn(x)
        assert len(calls) == 5
        monkeypatch.setattr(L, "flash_attention_available", lambda *a, **k: False)
        y_unfused = attn(x)
        assert len(calls) == 5
        attn.sliding_window = None
        y_nowin = attn(x)
        attn.sliding_window = 16
    rel = ((y_flash.float() - y_unfused.float()).abs().max()
           / (y_unfused.float().abs().max() + 1e-6)).item()
    assert rel < LAYER_TOL, f"windowed flash vs unfused layer mismatch {rel}"
    # the window must matter at this shape, or the comparison shows nothing
    assert (y_unfused.float() - y_nowin.float()).abs().max().item() > 0


def test_model_decode_step_matches_full_forward(monkeypatch):
    model = _tiny_windowed_llama()
    ids = torch.randint(0, 1024, (2, 40), device="cuda")
    fwd_calls = _record_ext(monkeypatch, "flash_fwd", 9)
    dec_calls = _record_ext(monkeypatch, "flash_decode", 6)
    with torch.no_grad():
        full = model(input_ids=ids)["prediction_scores"]
        o = model(input_ids=ids[:, :32], use_cache=True)
        # the windowed prompt pass runs the flash kernel too
        assert fwd_calls == [16] * 8, fwd_calls
        assert o["past_key_values"][0][0].shape == (2, 2, 32, 64)
        st = model(input_ids=ids[:, 32:33], past_key_values=o["past_key_values"],
                   use_cache=True)
    assert dec_calls == [16] * 4, dec_calls
    err = (o["prediction_scores"].float() - full[:, :32].float()).abs().max().item()
    assert err < LOGIT_TOL, err
    err = (st["prediction_scores"][:, 0].float() - full[:, 32].float()).abs().max()
    assert err.item() < LOGIT_TOL, err.item()


@torch.no_grad()
def _eager_greedy(model, prompt, n_new):
    out = model(input_ids=prompt, use_cache=True)
    past = out["past_key_values"]
    tok = out["prediction_scores"][:, -1, :].argmax(-1, keepdim=True)
    toks = [tok]
    for _ in range(n_new - 1):
        out = model(input_ids=tok, past_key_values=past, use_cache=True)
        past = out["past_key_values"]
        tok = out["prediction_scores"][:, -1, :].argmax(-1, keepdim=True)
        toks.append(tok)
    return torch.cat(toks, dim=1)


def test_captured_windowed_decode_matches_eager():
    from libai_amd.inference.captured_decode import CapturedLlamaDecoder

    model = _tiny_windowed_llama()
    b, L, n_new = 4, 32, 24
    prompt = torch.randint(0, 1024, (b, L), device="cuda")
    ref = _eager_greedy(model, prompt, n_new)
    for cap in (256, 1024):  # single-workgroup decode kernel / split path
        dec = CapturedLlamaDecoder(model, max_batch=b, max_seq_len=cap)
        got = dec.generate(prompt, n_new)
        assert torch.equal(got, ref), f"cap {cap} mismatch:\n{got}\nvs\n{ref}"


# 10. tile skipping really happens ---------------------------------------------------------
def test_window_tile_skipping_is_faster():
    """b1 h8 D64 S4096: window=128 visits about 6% of the causal tiles, so
    fwd+bwd must take less time than the windowless call."""
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(1, 4096, 8, 64, seed=7, grad=True)
    g = torch.randn(1, 4096, 8, 64, device="cuda", dtype=torch.bfloat16)

    def run(window):
        o = flash_attention(q, k, v, 0.125, causal=True, window=window)
        o.backward(g)
        q.grad = k.grad = v.grad = None

    def median_ms(window):
        times = []
        for it in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(window)
            torch.cuda.synchronize()
            if it >= 2:  # 2 warm-ups
                times.append((time.perf_counter() - t0) * 1e3)
        return sorted(times)[len(times) // 2]

    t_none = median_ms(None)
    t_win = median_ms(128)
    print(f"\nfwd+bwd b1 h8 D64 S4096: window=None {t_none:.3f} ms, "
          f"window=128 {t_win:.3f} ms ({t_none / t_win:.2f}x)")
    assert t_win < t_none
