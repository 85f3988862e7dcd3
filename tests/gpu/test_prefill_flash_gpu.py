"""The opt-in flash routes above the kernels: ``flash_prefill`` (prompt pass
with a cache, multi-token step on a past) for GPT, BLOOM and Llama, and
``flash_cross_attention`` for the T5 decoder."""

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYER_TOL = 3e-2  # flash vs unfused layer output, relative (test_flash_window_gpu.py)
LOGIT_TOL = 0.1   # cached pass vs full forward, model logits (same file)
LAYERS = 2
PROMPT, STEP = 35, 5  # a ragged past; PROMPT + STEP is a multiple of 8


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _gpt(flag):
    from libai_amd.models import GPTForPreTraining

    return GPTForPreTraining(hidden_layers=LAYERS, vocab_size=512, hidden_size=256,
                             ffn_hidden_size=512, num_attention_heads=4,
                             max_seq_length=64, flash_prefill=flag)


def _bloom(flag):
    from libai_amd.models.bloom import BloomForCausalLM

    return BloomForCausalLM(vocab_size=512, hidden_size=256, hidden_layers=LAYERS,
                            num_attention_heads=4, flash_prefill=flag)


def _llama(flag, window=None):
    from libai_amd.models.llama import LlamaForCausalLM

    return LlamaForCausalLM(hidden_layers=LAYERS, vocab_size=512, hidden_size=256,
                            intermediate_size=512, num_attention_heads=4,
                            num_key_value_heads=2, max_position_embeddings=64,
                            sliding_window=window, flash_prefill=flag)


def _llama_windowed(flag):
    return _llama(flag, window=16)


def _pair(build):
    torch.manual_seed(1)
    off = build(False).to("cuda", torch.bfloat16).eval()
    on = build(True).to("cuda", torch.bfloat16).eval()
    on.load_state_dict(off.state_dict())
    return off, on


def _record_routes(monkeypatch):
    """Record, in order, every flash_fwd call (with its q_offset) and every
    materialized-softmax call of the attention layers."""
    import libai_amd.layers.attention as LA
    import libai_amd.models.llama as LL
    import libai_amd.ops.softmax as S
    from libai_amd.ops._ext import ext

    calls = []
    orig_fwd = ext().flash_fwd

    def fwd(*a, **kw):
        calls.append(("flash_fwd", kw.get("q_offset", a[13] if len(a) > 13 else 0)))
        return orig_fwd(*a, **kw)

    monkeypatch.setattr(ext(), "flash_fwd", fwd)
    orig_sm = S.fused_scale_mask_softmax

    def softmax(*a, **kw):
        calls.append(("softmax", tuple(a[0].shape[-2:])))
        return orig_sm(*a, **kw)

    for mod in (S, LA, LL):
        monkeypatch.setattr(mod, "fused_scale_mask_softmax", softmax)
    return calls


@pytest.mark.parametrize("build", [_gpt, _bloom, _llama, _llama_windowed],
                         ids=["gpt", "bloom", "llama_gqa", "llama_window"])
def test_cached_passes_take_flash_and_match_full_forward(monkeypatch, build):
    off, on = _pair(build)
    ids = torch.randint(0, 512, (2, PROMPT + STEP), device="cuda")
    calls = _record_routes(monkeypatch)
    with torch.no_grad():
        full = off(input_ids=ids)["prediction_scores"]
        assert calls == [("flash_fwd", 0)] * LAYERS, calls
        # the caches of a causal pass over all the tokens (flag off)
        ref_cache = off(input_ids=ids, use_cache=True)["past_key_values"]
        del calls[:]

        # flag off: the parent's route, materialized scores in both passes
        p_off = off(input_ids=ids[:, :PROMPT], use_cache=True)
        assert calls == [("softmax", (PROMPT, PROMPT))] * LAYERS, calls
        del calls[:]
        s_off = off(input_ids=ids[:, PROMPT:], use_cache=True,
                    past_key_values=p_off["past_key_values"])
        assert calls == [("softmax", (STEP, PROMPT + STEP))] * LAYERS, calls
        del calls[:]

        # flag on: the flash forward, with the past length as the offset
        p_on = on(input_ids=ids[:, :PROMPT], use_cache=True)
        assert calls == [("flash_fwd", 0)] * LAYERS, calls
        del calls[:]
        s_on = on(input_ids=ids[:, PROMPT:], use_cache=True,
                  past_key_values=p_on["past_key_values"])
        assert calls == [("flash_fwd", PROMPT)] * LAYERS, calls

    for tag, got, want in (("prompt", p_on, full[:, :PROMPT]),
                           ("step", s_on, full[:, PROMPT:])):
        err = (got["prediction_scores"].float() - want.float()).abs().max().item()
        print(f"[prefill] {build.__name__} {tag} logits max abs err {err:.3e}")
        assert err < LOGIT_TOL, f"{tag}: {err}"

    # K and V do not depend on the route: the first layer, whose input is the
    # same in both models, caches the same bits.  Deeper layers see the other
    # route's activations: they agree within the layer tolerance with the
    # causal pass over the same tokens (the flag-off step is no reference
    # there: the materialized route does not mask among the new tokens).
    def rel_err(ta, tb):
        return ((ta.float() - tb.float()).abs().max() / tb.float().abs().max()).item()

    for tag, a, b, n in (("prompt", p_on, p_off, PROMPT),
                         ("step", s_on, s_off, PROMPT + STEP)):
        caches = zip(a["past_key_values"], b["past_key_values"], ref_cache)
        for i, (pa, pb, pr) in enumerate(caches):
            for ta, tb, tr in zip(pa, pb, pr):
                assert ta.shape == tb.shape and ta.dtype == tb.dtype
                if i == 0:
                    assert torch.equal(ta, tb), f"{tag} layer 0 cache differs"
                rel = rel_err(ta, tr[:, :, :n])
                assert rel < LAYER_TOL, f"{tag} layer {i} cache rel err {rel}"


@pytest.mark.parametrize("build", ["mha", "mha_alibi", "llama"])
def test_layer_caches_are_route_independent(build):
    """One attention layer, same input: the returned cache is bit-equal with
    the flag on and off, prompt pass and step."""
    from libai_amd.layers import MultiheadAttention
    from libai_amd.layers.position_bias import build_alibi_bias
    from libai_amd.models.llama import LlamaAttention

    init = torch.nn.init.xavier_normal_
    if build == "llama":
        def make(f):
            return LlamaAttention(256, 4, 64, init, init, num_key_value_heads=2,
                                  flash_prefill=f)
    else:
        def make(f):
            return MultiheadAttention(256, 4, attn_mask_type="causal",
                                      flash_prefill=f)
    off, on = _pair(make)
    x = torch.randn(2, PROMPT + STEP, 256, device="cuda", dtype=torch.bfloat16)

    def kw(n):
        if build != "mha_alibi":
            return {}
        return dict(position_bias=build_alibi_bias(4, n, device="cuda",
                                                   dtype=torch.bfloat16))

    with torch.no_grad():
        y0, c0 = off(x[:, :PROMPT], use_cache=True, **kw(PROMPT))
        y1, c1 = on(x[:, :PROMPT], use_cache=True, **kw(PROMPT))
        z0, d0 = off(x[:, PROMPT:], past_key_value=c0, use_cache=True,
                     **kw(PROMPT + STEP))
        z1, d1 = on(x[:, PROMPT:], past_key_value=c1, use_cache=True,
                    **kw(PROMPT + STEP))
    for a, b in zip(c0 + d0, c1 + d1):
        assert a.shape == b.shape and torch.equal(a, b)
    rel = ((y0.float() - y1.float()).abs().max() / y0.float().abs().max()).item()
    print(f"[prefill] {build} layer prompt rel err {rel:.3e}")
    assert rel < LAYER_TOL, rel


def test_short_chunk_on_long_cache_keeps_materialized_route(monkeypatch):
    """The class profiles/flash_prefill_cross.md measured slower is gated:
    a few workgroups walking a long cache."""
    from libai_amd.layers import MultiheadAttention

    off, on = _pair(lambda f: MultiheadAttention(256, 4, attn_mask_type="causal",
                                                 flash_prefill=f))
    past = tuple(torch.randn(1, 4, 4096, 64, device="cuda", dtype=torch.bfloat16)
                 for _ in range(2))
    x = torch.randn(1, 2, 256, device="cuda", dtype=torch.bfloat16)
    calls = _record_routes(monkeypatch)
    with torch.no_grad():
        y1 = on(x, past_key_value=past)
        assert calls == [("softmax", (2, 4098))], calls
        y0 = off(x, past_key_value=past)
    assert torch.equal(y0, y1)


def _decoder_layer(flag):
    from libai_amd.layers import TransformerLayer

    return TransformerLayer(256, 512, 4, is_decoder=True, attn_mask_type="causal",
                            flash_cross_attention=flag)


def test_t5_decoder_layer_cross_flash_matches_unfused(monkeypatch):
    import libai_amd.ops.attention as A
    from libai_amd.models.t5_model import cross_attn_mask

    torch.manual_seed(2)
    off = _decoder_layer(False).to("cuda", torch.bfloat16).train()
    on = _decoder_layer(True).to("cuda", torch.bfloat16).train()
    on.load_state_dict(off.state_dict())
    b, sq, sk = 2, 40, 64
    x = torch.randn(b, sq, 256, device="cuda", dtype=torch.bfloat16)
    enc = torch.randn(b, sk, 256, device="cuda", dtype=torch.bfloat16)
    enc_vis = torch.ones(b, sk, dtype=torch.uint8, device="cuda")
    enc_vis[1, 48:] = 0
    mask = cross_attn_mask(torch.ones(b, sq, dtype=torch.uint8, device="cuda"),
                           enc_vis)
    g = torch.randn_like(x)

    qkv_calls, kv_calls = [], []
    orig_qkv, orig_kv = A.flash_attention_qkv, A.flash_attention_kv
    monkeypatch.setattr(A, "flash_attention_qkv",
                        lambda *a, **k: (qkv_calls.append(1), orig_qkv(*a, **k))[1])
    monkeypatch.setattr(A, "flash_attention_kv",
                        lambda *a, **k: (kv_calls.append(k.get("kv_len")),
                                         orig_kv(*a, **k))[1])

    def run(layer):
        layer.zero_grad(set_to_none=True)
        n_qkv, n_kv = len(qkv_calls), len(kv_calls)
        y = layer(x, encoder_states=enc, encoder_attention_mask=mask)
        y.backward(g)
        ca = layer.cross_attention
        return (y.detach(), ca.query.weight.grad.clone(),
                ca.key_value.weight.grad.clone(), len(qkv_calls) - n_qkv,
                kv_calls[n_kv:])

    y0, dq0, dkv0, nq0, kv0 = run(off)
    y1, dq1, dkv1, nq1, kv1 = run(on)
    # the self-attention block's call only; the cross block goes its own way
    assert nq0 == 1 and nq1 == 1
    assert kv0 == [] and len(kv1) == 1 and kv1[0].tolist() == [64, 48]
    for name, a, b in (("out", y1, y0), ("dW query", dq1, dq0),
                       ("dW key_value", dkv1, dkv0)):
        rel = ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
        print(f"[cross-layer] {name} rel err {rel:.3e}")
        assert rel < LAYER_TOL, f"{name} rel err {rel}"
    assert dkv1.float().abs().max().item() > 0


@pytest.mark.parametrize("checkpoint", [False, True])
def test_t5_trains_one_step_through_cross_flash(monkeypatch, checkpoint):
    import libai_amd.ops.attention as A
    from libai_amd.models import T5ForPreTraining

    torch.manual_seed(0)
    layers_n, b, s_enc, s_dec, vocab = 2, 2, 64, 40, 512
    m = T5ForPreTraining(
        vocab_size=vocab, hidden_size=128, hidden_layers=layers_n,
        num_attention_heads=2, intermediate_size=256, max_position_embeddings=64,
        flash_cross_attention=True,
    ).to(torch.bfloat16).cuda().train()
    m.set_activation_checkpoint(checkpoint)
    enc_mask = torch.ones(b, s_enc, dtype=torch.uint8, device="cuda")
    enc_mask[1, 40:] = 0
    batch = dict(
        encoder_input_ids=torch.randint(0, vocab, (b, s_enc), device="cuda"),
        decoder_input_ids=torch.randint(0, vocab, (b, s_dec), device="cuda"),
        encoder_attn_mask=enc_mask,
        lm_labels=torch.randint(0, vocab, (b, s_dec), device="cuda"),
        loss_mask=torch.ones(b, s_dec, dtype=torch.long, device="cuda"),
    )
    calls = []
    orig = A.flash_attention_kv
    monkeypatch.setattr(A, "flash_attention_kv",
                        lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    loss = m(**batch)["masked_lm_loss"]
    assert len(calls) == layers_n
    loss.backward()
    assert len(calls) == (2 if checkpoint else 1) * layers_n
    assert torch.isfinite(loss).item()
    n_grads = 0
    for name, p in m.named_parameters():
        if p.grad is not None:
            n_grads += 1
            assert torch.isfinite(p.grad.float()).all(), name
    ca = m.t5_model.decoder_layers[0].cross_attention
    assert ca.key_value.weight.grad.float().abs().max().item() > 0
    assert n_grads > 0
