"""CPU side of the query offset and of the opt-in flash routes: argument
errors raised before the extension is touched, the ``_kv_len`` rule of
``cross_attn_mask``, and layers whose flags change nothing without a kernel."""

import pytest
import torch


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _qkv(sq=8, sk=24):
    q = torch.zeros(1, sq, 2, 64, dtype=torch.bfloat16)
    k = torch.zeros(1, sk, 2, 64, dtype=torch.bfloat16)
    return q, k, k.clone()


@pytest.mark.parametrize("kw,match", [
    (dict(q_offset=-1), ">= 0"),
    (dict(q_offset=16, causal=False), "causal"),
    (dict(q_offset=16, p_drop=0.1, training=True), "dropout"),
    (dict(q_offset=16, rel_bias=torch.zeros(2, 31)), "rel_bias"),
    (dict(q_offset=16, doc_bounds=(torch.zeros(1, 8, dtype=torch.int32),
                                   torch.zeros(1, 8, dtype=torch.int32))),
     "doc_bounds"),
    (dict(q_offset=17), "exceed"),
])
def test_q_offset_value_errors(kw, match):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv()
    with pytest.raises(ValueError, match=match):
        flash_attention(q, k, v, 0.125, **kw)


def test_q_offset_refuses_gradients():
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv()
    k.requires_grad_(True)
    with pytest.raises(ValueError, match="no backward"):
        flash_attention(q, k, v, 0.125, q_offset=16)


def test_eval_dropout_is_no_dropout_for_the_offset_rule():
    """p_drop with training=False is 0: the dropout rule must not fire (the
    call then fails only because there is no kernel on the CPU)."""
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv()
    with pytest.raises(Exception) as e:
        flash_attention(q, k, v, 0.125, p_drop=0.1, training=False, q_offset=16)
    assert "dropout" not in str(e.value)


def test_predicates_refuse_the_cpu():
    from libai_amd.ops.attention import flash_cross_available, flash_prefill_available

    cpu = torch.device("cpu")
    with torch.no_grad():
        assert not flash_prefill_available(64, torch.bfloat16, cpu, 5, 40)
    assert not flash_cross_available(64, torch.bfloat16, cpu, 40, 64, None)


def test_chunk_gate_keeps_few_workgroups_off_long_caches():
    from libai_amd.ops.attention import flash_chunk_pays

    assert flash_chunk_pays(2, 4, 5, 40)          # a short cache: always
    assert flash_chunk_pays(1, 32, 512, 2047)
    assert not flash_chunk_pays(1, 32, 16, 2064)  # 32 workgroups, long cache
    assert not flash_chunk_pays(1, 32, 16, 4112)
    assert not flash_chunk_pays(1, 32, 512, 4608)  # 128 workgroups
    assert flash_chunk_pays(1, 32, 513, 4609)     # 160 workgroups
    assert flash_chunk_pays(8, 32, 16, 4112)      # the batch fills the grid


def test_cross_attn_mask_attaches_kv_len_for_prefixes_only():
    from libai_amd.models.t5_model import cross_attn_mask

    dec = torch.tensor([[1, 1, 1], [1, 1, 0]])
    prefix = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]])
    m = cross_attn_mask(dec, prefix)
    assert m.shape == (2, 3, 4) and m.dtype == torch.uint8
    assert m._kv_len.dtype == torch.int32 and m._kv_len.tolist() == [4, 2]
    # the mask itself is the outer product it always was
    want = 1 - dec[:, :, None] * prefix[:, None, :]
    assert torch.equal(m, want.to(torch.uint8))
    for enc in (torch.tensor([[1, 0, 1, 1], [1, 1, 0, 0]]),
                torch.tensor([[0, 1, 1, 1], [1, 1, 1, 1]])):
        assert not hasattr(cross_attn_mask(dec, enc), "_kv_len")
    assert cross_attn_mask(None, prefix) is None


def _pair(build):
    torch.manual_seed(0)
    a = build(False)
    b = build(True)
    b.load_state_dict(a.state_dict())
    return a.eval(), b.eval()


def test_mha_flash_prefill_flag_is_inert_on_cpu():
    from libai_amd.layers import MultiheadAttention

    off, on = _pair(lambda f: MultiheadAttention(64, 2, attn_mask_type="causal",
                                                 flash_prefill=f))
    assert on.flash_prefill and not off.flash_prefill
    x = torch.randn(2, 12, 64)
    with torch.no_grad():
        y0, (k0, v0) = off(x[:, :8], use_cache=True)
        y1, (k1, v1) = on(x[:, :8], use_cache=True)
        assert torch.equal(y0, y1) and torch.equal(k0, k1) and torch.equal(v0, v1)
        z0 = off(x[:, 8:], past_key_value=(k0, v0))
        z1 = on(x[:, 8:], past_key_value=(k1, v1))
    assert torch.equal(z0, z1)


def test_mha_flash_cross_flag_is_inert_on_cpu():
    from libai_amd.layers import MultiheadAttention

    off, on = _pair(lambda f: MultiheadAttention(64, 2, is_cross_attention=True,
                                                 flash_cross_attention=f))
    x, enc = torch.randn(2, 5, 64), torch.randn(2, 8, 64)
    assert torch.equal(off(x, encoder_states=enc), on(x, encoder_states=enc))


def test_llama_flash_prefill_flag_is_inert_on_cpu():
    from libai_amd.models.llama import LlamaForCausalLM

    kw = dict(hidden_layers=2, vocab_size=64, hidden_size=64, intermediate_size=128,
              num_attention_heads=4, num_key_value_heads=2,
              max_position_embeddings=64)
    off, on = _pair(lambda f: LlamaForCausalLM(flash_prefill=f, **kw))
    assert on.model.layers[0].self_attn.flash_prefill
    ids = torch.randint(0, 64, (2, 12))
    with torch.no_grad():
        o0 = off(input_ids=ids[:, :8], use_cache=True)
        o1 = on(input_ids=ids[:, :8], use_cache=True)
        assert torch.equal(o0["prediction_scores"], o1["prediction_scores"])
        s0 = off(input_ids=ids[:, 8:], past_key_values=o0["past_key_values"])
        s1 = on(input_ids=ids[:, 8:], past_key_values=o1["past_key_values"])
    assert torch.equal(s0["prediction_scores"], s1["prediction_scores"])


def test_config_keys_default_off():
    from libai_amd.models import GPTModel, T5Model
    from libai_amd.models.bloom import BloomModel
    from libai_amd.models.llama import LlamaModel

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    base = Cfg(hidden_layers=1, vocab_size=64, hidden_size=64, ffn_hidden_size=128,
               intermediate_size=128, num_attention_heads=2)
    for cls in (GPTModel, BloomModel, LlamaModel):
        assert cls.from_config(base)["flash_prefill"] is False
        assert cls.from_config(Cfg(base, flash_prefill=True))["flash_prefill"] is True
    assert T5Model.from_config(base)["flash_cross_attention"] is False
    assert T5Model.from_config(Cfg(base, flash_cross_attention=True))[
        "flash_cross_attention"] is True
