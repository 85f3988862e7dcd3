"""CPU side of the split-KV forward: ``kv_split`` argument errors raised
before the extension is touched, and ``kv_split=None`` as the call it was."""

import inspect

import pytest
import torch


def _qkv(sq=8, sk=256):
    q = torch.zeros(1, sq, 2, 64, dtype=torch.bfloat16)
    k = torch.zeros(1, sk, 2, 64, dtype=torch.bfloat16)
    return q, k, k.clone()


_I32 = torch.zeros(1, 8, dtype=torch.int32)


@pytest.mark.parametrize("kw,match", [
    (dict(kv_split=128, p_drop=0.1, training=True), "dropout"),
    (dict(kv_split="auto", rel_bias=torch.zeros(2, 263)), "rel_bias"),
    (dict(kv_split=128, doc_bounds=(_I32, _I32)), "doc_bounds"),
    (dict(kv_split=100), "multiple of 128"),
    (dict(kv_split=0), "multiple of 128"),
])
def test_kv_split_value_errors(kw, match):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv()
    with pytest.raises(ValueError, match=match):
        flash_attention(q, k, v, 0.125, q_offset=248, **kw)


def test_kv_split_refuses_gradients():
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv()
    v.requires_grad_(True)
    with pytest.raises(ValueError, match="no backward"):
        flash_attention(q, k, v, 0.125, q_offset=248, kv_split=128)


def test_kv_split_none_is_the_call_it_was():
    """The default is None, and with None the rules of the other arguments
    fire as before (here: the query offset's)."""
    from libai_amd.ops.attention import flash_attention

    assert inspect.signature(flash_attention).parameters["kv_split"].default is None
    q, k, v = _qkv()
    with pytest.raises(ValueError, match="exceed"):
        flash_attention(q, k, v, 0.125, q_offset=249, kv_split=None)
    with pytest.raises(ValueError, match="causal"):
        flash_attention(q, k, v, 0.125, q_offset=8, causal=False, kv_split=None)
