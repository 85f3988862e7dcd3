"""Sliding-window (Mistral) attention on the unfused fp32 path: the Llama
model against a hand-written band-mask reference, incremental decode against
the full forward, config plumbing and argument validation."""

import math
import os
import types

import pytest
import torch

from libai_amd.utils import distributed as du

du.setup_dist_util({})

SEQ, W = 24, 5


def _model(sliding_window, seed=0):
    from libai_amd.models import LlamaForCausalLM

    torch.manual_seed(seed)
    return LlamaForCausalLM(
        hidden_layers=2, vocab_size=128, hidden_size=64, intermediate_size=128,
        num_attention_heads=4, num_key_value_heads=2,
        max_position_embeddings=64, sliding_window=sliding_window,
    ).eval()


def _ref_attention(attn, x, window):
    """Hand-written fp32 attention of one LlamaAttention module: its own
    projections and RoPE, then softmax over an explicit -inf band mask."""
    from libai_amd.ops.rope import apply_rotary_pos_emb

    b, s, _ = x.shape
    q, k, v = attn._project(x)
    q = apply_rotary_pos_emb(q, attn.max_pos, attn.rope_theta, 0)
    k = apply_rotary_pos_emb(k, attn.max_pos, attn.rope_theta, 0)
    group = attn.num_heads // attn.num_kv_heads
    qh = q.permute(0, 2, 1, 3)
    kh = k.permute(0, 2, 1, 3).repeat_interleave(group, dim=1)
    vh = v.permute(0, 2, 1, 3).repeat_interleave(group, dim=1)
    scores = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(attn.head_dim)
    i = torch.arange(s)[:, None]
    j = torch.arange(s)[None, :]
    visible = (j <= i) & (i - j < window)
    scores = scores.masked_fill(~visible, float("-inf"))
    ctx = torch.matmul(torch.softmax(scores, dim=-1), vh)
    out, _ = attn.o_proj(ctx.permute(0, 2, 1, 3).reshape(b, s, -1))
    return out


def test_attention_module_matches_band_mask_reference():
    m = _model(W)
    attn = m.model.layers[0].self_attn
    assert attn.sliding_window == W
    torch.manual_seed(1)
    x = torch.randn(2, SEQ, 64)
    with torch.no_grad():
        got = attn(x)
        want = _ref_attention(attn, x, W)
        full = _ref_attention(attn, x, SEQ)
    assert (got - want).abs().max().item() < 1e-5
    # the window must matter at this shape, or the check shows nothing
    assert (want - full).abs().max().item() > 1e-3


def test_model_logits_match_band_mask_reference():
    m = _model(W)
    ids = torch.randint(0, 128, (2, SEQ), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        got = m(input_ids=ids)["prediction_scores"]
        # same weights, every attention module replaced by the reference
        for layer in m.model.layers:
            attn = layer.self_attn

            def ref_forward(self, hidden_states, past_key_value=None,
                            use_cache=False, residual=None, static_cache=None,
                            position=None):
                return _ref_attention(self, hidden_states, W) + residual

            attn.forward = types.MethodType(ref_forward, attn)
        want = m(input_ids=ids)["prediction_scores"]
        plain = _model(None)(input_ids=ids)["prediction_scores"]
    assert (got - want).abs().max().item() < 1e-4
    assert (got - plain).abs().max().item() > 1e-3


@pytest.mark.parametrize("window", [SEQ, SEQ + 7])
def test_full_length_window_equals_no_window(window):
    ids = torch.randint(0, 128, (2, SEQ), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        a = _model(window)(input_ids=ids)["prediction_scores"]
        b = _model(None)(input_ids=ids)["prediction_scores"]
    assert torch.equal(a, b)


def test_incremental_decode_matches_full_forward():
    prompt, steps = 12, 8  # W=5 < prompt: the prefill and every step clip
    m = _model(W)
    ids = torch.randint(0, 128, (2, prompt + steps),
                        generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        full = m(input_ids=ids)["prediction_scores"]
        out = m(input_ids=ids[:, :prompt], use_cache=True)
        assert torch.allclose(out["prediction_scores"], full[:, :prompt], atol=1e-5)
        past = out["past_key_values"]
        for t in range(prompt, prompt + steps):
            out = m(input_ids=ids[:, t:t + 1], past_key_values=past, use_cache=True)
            past = out["past_key_values"]
            # the cache keeps every key; the window only masks
            assert past[0][0].shape[2] == t + 1
            err = (out["prediction_scores"][:, 0] - full[:, t]).abs().max().item()
            assert err < 1e-5, (t, err)
        # and the window is what makes them agree: without it the step differs
        plain = _model(None)
        o2 = plain(input_ids=ids[:, :prompt], use_cache=True)
        s2 = plain(input_ids=ids[:, prompt:prompt + 1],
                   past_key_values=o2["past_key_values"], use_cache=True)
        assert (s2["prediction_scores"][:, 0] - full[:, prompt]).abs().max() > 1e-3


def test_from_config_builds_windowed_model():
    from libai_amd.config import ConfigDict
    from libai_amd.models import LlamaForCausalLM

    base = dict(hidden_layers=1, vocab_size=64, hidden_size=64,
                intermediate_size=128, num_attention_heads=4)
    m = LlamaForCausalLM(ConfigDict(dict(base, sliding_window=7)))
    assert m.model.sliding_window == 7
    assert all(l.self_attn.sliding_window == 7 for l in m.model.layers)
    m0 = LlamaForCausalLM(ConfigDict(base))
    assert m0.model.layers[0].self_attn.sliding_window is None


def test_mistral_recipe_carries_sliding_window():
    from libai_amd.config import LazyConfig

    cfg = LazyConfig.load(os.path.join(os.path.dirname(__file__), "..", "configs",
                                       "mistral_7b_pretrain.py"))
    assert cfg.model.sliding_window == 4096
    assert cfg.model.num_key_value_heads == 8
    assert cfg.model.hidden_layers == 32 and cfg.model.hidden_size == 4096
    assert cfg.model.intermediate_size == 14336 and cfg.model.vocab_size == 32000
    assert cfg.model.max_position_embeddings == 8192


def test_window_argument_validation():
    from libai_amd.ops.attention import (
        flash_attention,
        flash_attention_qkv,
        flash_decode_attn,
    )

    q = torch.randn(1, 16, 2, 64)
    slopes = torch.ones(2)
    with pytest.raises(ValueError, match="alibi"):
        flash_attention(q, q, q, 0.125, causal=True, alibi_slopes=slopes, window=4)
    with pytest.raises(ValueError, match="causal"):
        flash_attention(q, q, q, 0.125, causal=False, window=4)
    with pytest.raises(ValueError, match="window"):
        flash_attention(q, q, q, 0.125, causal=True, window=-1)
    qkv = torch.randn(1, 16, 2, 3, 64)
    with pytest.raises(ValueError, match="causal"):
        flash_attention_qkv(qkv, 0.125, causal=False, window=4)
    qd = torch.randn(1, 2, 1, 64)
    kd = torch.randn(1, 2, 16, 64)
    with pytest.raises(ValueError, match="alibi"):
        flash_decode_attn(qd, kd, kd, 0.125, alibi_slopes=slopes, window=4)
