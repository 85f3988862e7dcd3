"""ALiBi slope plumbing (CPU): the fp32 slopes ride on the bias tensor and
the CPU attention path ignores them."""

import pytest
import torch

from libai_amd.utils import distributed as du

du.setup_dist_util({})


@pytest.mark.parametrize("n", [4, 6, 8, 16])
def test_local_alibi_slopes_equals_global_at_tp1(n):
    from libai_amd.layers.position_bias import alibi_slopes, local_alibi_slopes

    local = local_alibi_slopes(n, device="cpu")
    assert local.dtype == torch.float32 and local.is_contiguous()
    assert local.shape == (n,)
    assert torch.equal(local, alibi_slopes(n).to(torch.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_build_alibi_bias_attaches_fp32_slopes(dtype):
    from libai_amd.layers.position_bias import build_alibi_bias
    from libai_amd.ops.attention import bias_alibi_slopes

    bias = build_alibi_bias(8, 16, device="cpu", dtype=dtype)
    assert bias.shape == (8, 1, 16) and bias.dtype == dtype
    slopes = bias_alibi_slopes(bias)
    assert slopes is not None and slopes is bias._alibi_slopes
    assert slopes.dtype == torch.float32 and slopes.shape == (8,)
    # slope_h == bias[h, 0, 1] (key position 1), computed in fp32
    ref = build_alibi_bias(8, 16, device="cpu", dtype=torch.float32)[:, 0, 1]
    assert torch.equal(slopes, ref)
    # biases from anywhere else carry no slopes
    assert bias_alibi_slopes(torch.zeros(8, 1, 16)) is None
    assert bias_alibi_slopes(None) is None


def test_bloom_alibi_cache_keeps_slopes():
    from libai_amd.models.bloom import BloomModel

    m = BloomModel(vocab_size=64, hidden_size=32, hidden_layers=1,
                   num_attention_heads=4)
    b1 = m.alibi(12, torch.device("cpu"), torch.float32)
    b2 = m.alibi(12, torch.device("cpu"), torch.float32)
    assert b1 is b2  # cached object, attribute included
    assert getattr(b2, "_alibi_slopes", None) is not None
    assert b2._alibi_slopes.dtype == torch.float32
    assert b2._alibi_slopes.numel() == 4


def test_cpu_layer_ignores_slopes_attribute():
    """On CPU there is no fused kernel: a bias with slopes and the same
    tensor without them give identical results, cache path included."""
    from libai_amd import layers
    from libai_amd.layers.position_bias import build_alibi_bias

    torch.manual_seed(0)
    attn = layers.MultiheadAttention(32, 4, attn_mask_type="causal").eval()
    x = torch.randn(2, 12, 32)
    bias = build_alibi_bias(4, 12, device="cpu")
    plain = bias.clone()
    assert getattr(plain, "_alibi_slopes", None) is None
    with torch.no_grad():
        assert torch.equal(attn(x, position_bias=bias),
                           attn(x, position_bias=plain))
        # single-token decode against a cache
        _, (k, v) = attn(x[:, :11], position_bias=build_alibi_bias(4, 11),
                         use_cache=True)
        y1 = attn(x[:, 11:], position_bias=bias, past_key_value=(k, v))
        y2 = attn(x[:, 11:], position_bias=plain, past_key_value=(k, v))
        assert torch.equal(y1, y2)
