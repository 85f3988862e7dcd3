"""The diagonal table T5RelativePositionBias attaches to its bias: the bias is
Toeplitz, bias[0, h, i, j] == table[h, j - i + sq - 1], and the table carries
the gradient back to the bucket weight.  CPU only: the kernels that consume
the table are tested in tests/gpu/test_flash_relbias_gpu.py."""

import pytest
import torch

from libai_amd.utils import distributed as du

du.setup_dist_util({})

NH = 4


def _module(bidirectional, seed=0):
    from libai_amd.layers.position_bias import T5RelativePositionBias

    torch.manual_seed(seed)
    return T5RelativePositionBias(NH, num_buckets=32, max_distance=128,
                                  bidirectional=bidirectional)


def _diag_index(sq, sk):
    i = torch.arange(sq)[:, None]
    j = torch.arange(sk)[None, :]
    return j - i + (sq - 1)


@pytest.mark.parametrize("bidirectional", [True, False])
@pytest.mark.parametrize("sq,sk", [(8, 8), (40, 40), (200, 200)])
def test_table_is_the_bias_diagonal_by_diagonal(bidirectional, sq, sk):
    from libai_amd.ops.attention import bias_rel_table

    m = _module(bidirectional)
    bias = m(sq, sk)
    table = bias_rel_table(bias)
    assert table is not None and table is bias._rel_bias_table
    assert bias.shape == (1, NH, sq, sk)
    assert table.dtype == torch.float32 and table.is_contiguous()
    assert table.shape == (NH, sq + sk - 1)
    assert table.requires_grad
    # every (i, j), exactly
    assert torch.equal(bias[0].float(), table[:, _diag_index(sq, sk)])
    # the bias values themselves are what the bucket gather gives
    rel = torch.arange(sk)[None, :] - torch.arange(sq)[:, None]
    buckets = m._bucket(rel, bidirectional, m.num_buckets, m.max_distance)
    assert torch.equal(bias[0], m.weight[buckets].permute(2, 0, 1))


@pytest.mark.parametrize("bidirectional", [True, False])
def test_table_gradient_reaches_the_weight(bidirectional):
    sq = sk = 40
    m = _module(bidirectional, seed=1)
    bias = m(sq, sk)
    bias._rel_bias_table.sum().backward()
    got = m.weight.grad.clone()
    m.weight.grad = None
    # one representative (i, j) per diagonal of the materialized bias: row 0
    # holds the deltas 0 .. sk-1, column 0 the deltas -(sq-1) .. -1
    bias2 = m(sq, sk)
    (bias2[0, :, 0, :].sum() + bias2[0, :, 1:, 0].sum()).backward()
    assert torch.equal(got, m.weight.grad)
    assert got.abs().sum().item() > 0


def test_table_in_half_precision_weight_is_exact():
    m = _module(True).to(torch.bfloat16)
    bias = m(24, 24)
    table = bias._rel_bias_table
    assert bias.dtype == torch.bfloat16 and table.dtype == torch.float32
    assert torch.equal(bias[0].float(), table[:, _diag_index(24, 24)])


def test_bias_rel_table_none_cases():
    from libai_amd.ops.attention import bias_rel_table

    assert bias_rel_table(None) is None
    assert bias_rel_table(torch.zeros(1, NH, 8, 8)) is None
    # a slice of the bias (the cached-decode form) is a plain tensor again
    bias = _module(False)(16, 16)
    assert bias_rel_table(bias[:, :, 8:, :]) is None


def test_op_rejects_table_with_slopes_or_window():
    from libai_amd.ops.attention import flash_attention, flash_attention_qkv

    s, d = 16, 64
    q = torch.zeros(1, s, NH, d, dtype=torch.bfloat16)
    qkv = torch.zeros(1, s, NH, 3, d, dtype=torch.bfloat16)
    table = torch.zeros(NH, 2 * s - 1)
    slopes = torch.ones(NH)
    with pytest.raises(ValueError, match="alibi_slopes"):
        flash_attention(q, q, q, 0.125, causal=True, alibi_slopes=slopes,
                        rel_bias=table)
    with pytest.raises(ValueError, match="window"):
        flash_attention(q, q, q, 0.125, causal=True, window=4, rel_bias=table)
    with pytest.raises(ValueError, match="alibi_slopes"):
        flash_attention_qkv(qkv, 0.125, causal=True, alibi_slopes=slopes,
                            rel_bias=table)
    with pytest.raises(ValueError, match="window"):
        flash_attention_qkv(qkv, 0.125, causal=True, window=4, rel_bias=table)
