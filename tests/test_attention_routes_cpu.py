"""The attention layers' decision, asked without a GPU: every row of
``tests/attention_route_cases.py`` as a GPU-shaped call (``torch.device("cuda")``
and bf16 passed as values, no tensor placed there) must get the route whose
kernels ``tests/gpu/test_attention_routes_gpu.py`` sees the call reach, and
the same calls on the CPU must all get the materialized / unfused route."""

import pytest
import torch

from tests.attention_route_cases import (CASE_IDS, CASES, build_bias, build_layer,
                                         build_mask, key_count)

# the entry points a route reaches first, or "softmax" for the materialized one
ROUTE_KERNEL = {
    "flash_qkv": "flash_fwd", "flash_cross": "flash_fwd", "flash_prompt": "flash_fwd",
    "flash": "flash_fwd", "flash_chunk": "flash_fwd",
    "flash_chunk_split": "flash_fwd_split", "decode": "flash_decode",
    "materialized": "softmax", "unfused": "softmax",
}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _split_keys_auto(batch, kv_heads, kv_group, sq, sk):
    """``flash_split_keys_auto`` of csrc/kernels/flash_attn.hip, transcribed:
    the extension is not built on machines without a GPU toolchain."""
    def cdiv(a, b):
        return -(-a // b)

    if min(batch, kv_heads, kv_group, sq, sk) <= 0:
        return 0
    tiles = batch * kv_heads * cdiv(kv_group * sq, 128)
    if batch > 1 or sk < 1024 or tiles > 128:
        return 0
    if kv_group * sq < 32 and tiles * sk > 32 * 2064:
        return 0
    keys = cdiv(cdiv(sk, cdiv(512, tiles)), 128) * 128
    return max(keys, 128)


def _decide(case, device, monkeypatch):
    import libai_amd.ops.attention as A

    monkeypatch.setattr(A, "flash_split_keys", _split_keys_auto)
    layer = build_layer(case)
    kw = dict(has_past=bool(case["past"]) or case["cross_past"],
              use_cache=case["use_cache"])
    if case["layer"] != "llama":
        kw.update(attention_mask=build_mask(case, "cpu"),
                  position_bias=build_bias(case, "cpu", torch.bfloat16))
    with torch.set_grad_enabled(case["grad"]):
        return layer._route(case["batch"], case["sq"], key_count(case),
                            torch.bfloat16, torch.device(device), **kw)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decision_on_gpu_shaped_call(monkeypatch, case):
    route = _decide(case, "cuda", monkeypatch)
    assert route == case["route"]
    # the table agrees with itself: the route's kernel is the one expected first
    first = case["expect"][0][0]
    assert ROUTE_KERNEL[route] == ("softmax" if first.startswith("softmax") else first)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decision_on_cpu_is_materialized(monkeypatch, case):
    want = "unfused" if case["layer"] == "llama" else "materialized"
    assert _decide(case, "cpu", monkeypatch) == want


@pytest.mark.parametrize("layer", ["mha", "llama"])
def test_static_cache_is_decided_first(monkeypatch, layer):
    case = next(c for c in CASES if c["layer"] == layer)
    route = build_layer(case)._route(2, 1, 1, torch.bfloat16, torch.device("cuda"),
                                     static_cache=True)
    assert route == "static_decode"


def test_split_policy_transcription_matches_extension():
    """Where the extension is built, the transcription above is checked
    against it on the shapes around each of its gates."""
    from libai_amd.ops._ext import ext, has_ext

    if not has_ext():
        pytest.skip("extension not built")
    for b in (1, 2):
        for hkv, g in ((2, 1), (2, 2), (8, 4), (32, 1)):
            for sq in (1, 15, 16, 31, 32, 128, 512, 4096):
                for sk in (1023, 1024, 2064, 2080, 4096, 33025):
                    assert _split_keys_auto(b, hkv, g, sq, sk) == \
                        ext().flash_split_keys_auto(b, hkv, g, sq, sk), (b, hkv, g, sq, sk)
