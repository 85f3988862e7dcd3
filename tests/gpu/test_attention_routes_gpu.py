"""Which kernels a call of ``MultiheadAttention`` / ``LlamaAttention`` reaches.

Every row of ``tests/attention_route_cases.py`` runs once; the entry points of
the extension it reaches are recorded by wrapping the attributes of ``ext()``
(``flash_fwd`` with its ``q_offset``, ``flash_fwd_split``, ``flash_bwd``,
``flash_decode``, ``softmax_fwd``), never a Python name of the layer modules.
Score widths that are no multiple of 8 leave ``softmax_fwd`` for the composed
softmax of ``ops/softmax.py``; that one is recorded too, as the only trace of
the materialized route at such a width.

Rows that differ only in ``flash_prefill`` must return the same cache, bit for
bit: the cached K and V are the same projections whichever kernel reads them.
Outputs of different routes are not compared here (different kernels round
differently; ``test_prefill_flash_gpu.py`` bounds that difference).
"""

import pytest
import torch

from tests.attention_route_cases import (CASE_IDS, CASES, HEAD_DIM, LLAMA_HIDDEN,
                                         LLAMA_KV_HEADS, MHA_HEADS, MHA_HIDDEN, PAIRS,
                                         build_bias, build_docs, build_layer,
                                         build_mask)

pytestmark = pytest.mark.gpu

DTYPE = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _spy(monkeypatch):
    """Record, in order, the extension entry points a call reaches."""
    import libai_amd.ops.softmax as S
    from libai_amd.ops._ext import ext

    calls = []

    def wrap(owner, name, describe):
        orig = getattr(owner, name)

        def wrapper(*a, **kw):
            calls.append(describe(a, kw))
            return orig(*a, **kw)

        monkeypatch.setattr(owner, name, wrapper)

    def arg(a, kw, name, pos):
        return kw.get(name, a[pos] if len(a) > pos else 0)

    wrap(ext(), "flash_fwd", lambda a, kw: ("flash_fwd", arg(a, kw, "q_offset", 13)))
    wrap(ext(), "flash_fwd_split",
         lambda a, kw: ("flash_fwd_split", arg(a, kw, "q_offset", 8)))
    wrap(ext(), "flash_bwd", lambda a, kw: ("flash_bwd",))
    wrap(ext(), "flash_decode", lambda a, kw: ("flash_decode",))
    wrap(ext(), "softmax_fwd", lambda a, kw: ("softmax_fwd", tuple(a[0].shape[-2:])))
    wrap(S, "_ref", lambda a, kw: ("softmax_composed", tuple(a[0].shape[-2:])))
    return calls


def _inputs(case):
    gen = torch.Generator().manual_seed(3)

    def rand(*shape):
        return torch.randn(*shape, generator=gen).to("cuda", DTYPE)

    b, sq = case["batch"], case["sq"]
    if case["layer"] == "llama":
        kw = dict(hidden_states=rand(b, sq, LLAMA_HIDDEN))
        heads = LLAMA_KV_HEADS
        docs = build_docs(case, "cuda")
        if docs is not None:
            kw.update(doc_start=docs[0], doc_end=docs[1])
    else:
        kw = dict(hidden_states=rand(b, sq, MHA_HIDDEN),
                  attention_mask=build_mask(case, "cuda"),
                  position_bias=build_bias(case, "cuda", DTYPE))
        heads = MHA_HEADS
        if case["layer"] == "cross":
            kw["encoder_states"] = rand(b, case["sk_enc"], MHA_HIDDEN)
            if case["cross_past"]:
                kw["past_key_value"] = (rand(b, heads, case["sk_enc"], HEAD_DIM),
                                        rand(b, heads, case["sk_enc"], HEAD_DIM))
    if case["past"]:
        kw["past_key_value"] = (rand(b, heads, case["past"], HEAD_DIM),
                                rand(b, heads, case["past"], HEAD_DIM))
    if case["use_cache"]:
        kw["use_cache"] = True
    return kw


_RESULTS = {}


def _run(case, monkeypatch):
    """(entry points reached, output, cache) of a row; each row runs once."""
    if case["id"] not in _RESULTS:
        layer = build_layer(case).to("cuda", DTYPE)
        kw = _inputs(case)
        calls = _spy(monkeypatch)
        with torch.set_grad_enabled(case["grad"]):
            out = layer(**kw)
            present = None
            if case["use_cache"]:
                out, present = out
            if case["backward"]:
                out.float().square().mean().backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        _RESULTS[case["id"]] = (list(calls), out.detach(), present)
    return _RESULTS[case["id"]]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_call_reaches_expected_kernels(monkeypatch, case):
    calls, out, present = _run(case, monkeypatch)
    print(f"[routes] {case['id']}: {calls}")
    assert calls == case["expect"], (case["id"], calls)
    assert out.shape[:2] == (case["batch"], case["sq"])
    assert torch.isfinite(out.float()).all()
    assert (present is not None) == case["use_cache"]


@pytest.mark.parametrize("pair", PAIRS)
def test_cache_is_bit_equal_across_flag(monkeypatch, pair):
    rows = [c for c in CASES if c["pair"] == pair]
    assert len(rows) == 2
    (_, _, cache_a), (_, _, cache_b) = (_run(c, monkeypatch) for c in rows)
    assert cache_a is not None and cache_b is not None
    for ta, tb in zip(cache_a, cache_b):
        assert ta.shape == tb.shape and ta.dtype == tb.dtype
        assert torch.equal(ta, tb), f"{pair}: cache differs between {rows[0]['id']} " \
                                    f"and {rows[1]['id']}"
