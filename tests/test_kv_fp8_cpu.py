"""FP8 KV cache: what the ops layer decides without a GPU."""
import pytest
import torch

from libai_amd.ops.attention import decode_fp8_available, flash_decode_attn_fp8
from libai_amd.ops.kv_cache import alloc_fp8_cache, dequantize


def _args(h=8, kvh=2, d=64, cap=16, scale_cap=None):
    q = torch.zeros(1, h, 1, d, dtype=torch.bfloat16)
    k8 = torch.zeros(1, kvh, cap, d, dtype=torch.uint8)
    ks = torch.ones(1, kvh, scale_cap or cap)
    return q, k8, k8.clone(), ks, ks.clone(), d ** -0.5


@pytest.mark.parametrize("kwargs, extra", [
    (dict(h=18, kvh=2), {}),                                 # G = 9 > 8
    (dict(d=96), {}),                                        # head size 96
    (dict(scale_cap=15), {}),                                # scale shape mismatch
    (dict(), dict(alibi_slopes=torch.ones(8))),              # no ALiBi form
])
def test_wrapper_rejects(kwargs, extra):
    with pytest.raises(ValueError):
        flash_decode_attn_fp8(*_args(**kwargs), **extra)


def test_available():
    assert decode_fp8_available(64, 1) and decode_fp8_available(128, 8)
    assert not decode_fp8_available(128, 9) and not decode_fp8_available(96, 4)


def test_alloc_shapes_and_dtypes():
    c8, scale = alloc_fp8_cache(3, 2, 40, 128, "cpu")
    assert c8.shape == (3, 2, 40, 128) and c8.dtype == torch.uint8
    assert scale.shape == (3, 2, 40) and scale.dtype == torch.float32
    assert int(c8.max()) == 0 and bool((scale == 1).all())
    with pytest.raises(ValueError):
        alloc_fp8_cache(1, 1, 8, 96, "cpu")


def test_dequantize_round_trip():
    # the format's rule in torch; half an e4m3 ulp is 2^-4 relative, its
    # subnormals are 2^-9 apart
    torch.manual_seed(0)
    x = (torch.randn(2, 2, 33, 64) * torch.exp2(torch.randn(2, 2, 33, 1) * 3))
    x = x.bfloat16().float()
    scale = x.abs().amax(-1) / 448.0
    c8 = (x / scale[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    deq = dequantize(c8.view(torch.uint8), scale)
    bound = x.abs() * 2.0 ** -4 + scale[..., None] * 2.0 ** -10
    assert bool(((deq - x).abs() <= bound).all())
