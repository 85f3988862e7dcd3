"""window_attention's argument checks and the layer's fallback (no GPU)."""

import pytest
import torch


def _args(n=49, h=3, b_=4, d=32, nw=None, bias_dtype=torch.float32):
    qkv = torch.zeros(b_, n, 3, h, d, dtype=torch.bfloat16)
    bias = torch.zeros(h, n, n, dtype=bias_dtype)
    mask = None if nw is None else torch.zeros(nw, n, n)
    return qkv, bias, mask


@pytest.mark.parametrize("kw", [
    dict(d=64),                       # head size
    dict(n=65),                       # tokens per window
    dict(b_=4, nw=3),                 # B_ not a multiple of nW
    dict(bias_dtype=torch.bfloat16),  # bias must be fp32
])
def test_window_attention_rejects(kw):
    from libai_amd.ops.attention import window_attention

    qkv, bias, mask = _args(**kw)
    with pytest.raises(ValueError):
        window_attention(qkv, bias, 32 ** -0.5, mask=mask)


def test_fused_flag_falls_back_on_cpu():
    from libai_amd.models.swin_transformer import WindowAttention

    torch.manual_seed(0)
    base = WindowAttention(96, 7, 3)
    fused = WindowAttention(96, 7, 3, fused_window_attention=True)
    fused.load_state_dict(base.state_dict())
    x = torch.randn(8, 49, 96)
    mask = torch.where(torch.rand(4, 49, 49) < 0.3, -100.0, 0.0)
    assert torch.equal(fused(x, mask=mask), base(x, mask=mask))
