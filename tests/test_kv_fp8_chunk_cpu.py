"""Multi-token steps on the FP8 KV cache: what is decided without a GPU."""
import pytest
import torch

from libai_amd.ops import attention
from libai_amd.ops.kv_cache import accept_greedy


@pytest.mark.parametrize("draft, target, n, nxt", [
    ([[5, 6, 7]], [[5, 6, 7, 8]], [3], [8]),        # all match: the bonus token
    ([[5, 6, 7]], [[4, 6, 7, 8]], [0], [4]),        # first wrong
    ([[5, 6, 7]], [[5, 9, 7, 8]], [1], [9]),        # a match after a mismatch
    ([[5]], [[5, 2]], [1], [2]),                    # K = 1, accepted
    ([[5], [3]], [[1, 2], [3, 4]], [0, 1], [1, 4]),  # K = 1, per row
])
def test_accept_greedy(draft, target, n, nxt):
    got_n, got_next = accept_greedy(torch.tensor(draft), torch.tensor(target))
    assert got_n.tolist() == n and got_next.tolist() == [[x] for x in nxt]


def _args(t, h=8, kvh=2, d=64, cap=16):
    q = torch.zeros(1, h, t, d, dtype=torch.bfloat16)
    k8 = torch.zeros(1, kvh, cap, d, dtype=torch.uint8)
    ks = torch.ones(1, kvh, cap)
    return q, k8, k8.clone(), ks, ks.clone(), d ** -0.5


def test_wrapper_rejects_33_tokens():
    with pytest.raises(ValueError):
        attention.flash_decode_attn_fp8(*_args(33))


@pytest.mark.parametrize("t, binding", [(1, "flash_decode_fp8"),
                                        (2, "flash_chunk_fp8"),
                                        (32, "flash_chunk_fp8")])
def test_wrapper_picks_binding(monkeypatch, t, binding):
    called = []

    class Ext:
        def __getattr__(self, name):
            return lambda *a: called.append(name)

    monkeypatch.setattr(attention, "ext", Ext)
    attention.flash_decode_attn_fp8(*_args(t))
    assert called == [binding]
