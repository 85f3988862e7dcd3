"""The calls that pin the routes of ``MultiheadAttention`` and ``LlamaAttention``.

One table, two readers: ``tests/gpu/test_attention_routes_gpu.py`` runs every
row on the GPU and records the extension entry points the call reaches;
``tests/test_attention_routes_cpu.py`` asks the layers' decision for the same
rows without a GPU.  Nothing here needs one.

Shapes: MHA hidden 128, 2 heads of 64, causal unless cross; Llama attention
hidden 256, 4 query heads on 2 KV heads of 64.  They are the smallest at which
every predicate can still go either way: ``sk % 8``, a ragged prompt,
``sq > 1``, the 2048-key and 128-workgroup gates of ``flash_chunk_pays`` and
the batch-1 gate of the split-KV policy.

``expect``: the entry points of the extension a call reaches, in order.  The
materialized route reaches ``softmax_fwd`` only where the key count is a
multiple of 8; other widths run the composed softmax of ``ops/softmax.py``
(``softmax_composed``), which is no entry point of the extension but is the
only trace such a call leaves.
``route``: the name the layer's decision gives the call.
``pair``: rows of one pair differ in a flag only and must cache the same bits.
"""

import torch

MHA_HIDDEN, MHA_HEADS = 128, 2
LLAMA_HIDDEN, LLAMA_HEADS, LLAMA_KV_HEADS, LLAMA_MAX_POS = 256, 4, 2, 4096
HEAD_DIM = 64

FLASH0 = ("flash_fwd", 0)
FLASH_BWD = ("flash_bwd",)
DECODE = ("flash_decode",)


def softmax(sq, sk):
    """What the materialized route leaves behind on [.., sq, sk] scores."""
    return ("softmax_fwd" if sk % 8 == 0 else "softmax_composed", (sq, sk))


def _case(id, layer, expect, route, *, ctor=None, batch=2, sq=16, past=0,
          sk_enc=None, use_cache=False, train_mode=False, grad=False,
          backward=False, bias=None, mask=None, docs=None, cross_past=False,
          pair=None):
    return dict(id=id, layer=layer, expect=list(expect), route=route,
                ctor=dict(ctor or {}), batch=batch, sq=sq, past=past,
                sk_enc=sk_enc, use_cache=use_cache, train_mode=train_mode,
                grad=grad, backward=backward, bias=bias, mask=mask, docs=docs,
                cross_past=cross_past, pair=pair)


def _prefill(flag):
    return dict(flash_prefill=flag)


def _cross(flag):
    return dict(flash_cross_attention=flag)


CASES = [
    # -- MultiheadAttention, causal self-attention ---------------------------
    _case("mha-train-s16", "mha", [FLASH0, FLASH_BWD], "flash_qkv",
          train_mode=True, grad=True, backward=True),
    _case("mha-s12", "mha", [softmax(12, 12)], "materialized", sq=12),
    _case("mha-s16-plain-bias", "mha", [softmax(16, 16)], "materialized",
          bias="plain"),
    _case("mha-s16-alibi", "mha", [FLASH0], "flash_qkv", bias="alibi"),
    _case("mha-s16-mask-kvlen", "mha", [FLASH0], "flash_qkv", mask="kv_len"),
    _case("mha-s16-mask-plain", "mha", [softmax(16, 16)], "materialized",
          mask="plain"),
    _case("mha-prompt13-off", "mha", [softmax(13, 13)], "materialized", sq=13,
          use_cache=True, ctor=_prefill(False), pair="mha-prompt13"),
    _case("mha-prompt13-on", "mha", [FLASH0], "flash_prompt", sq=13,
          use_cache=True, ctor=_prefill(True), pair="mha-prompt13"),
    _case("mha-prompt13-on-grad", "mha", [softmax(13, 13)], "materialized",
          sq=13, use_cache=True, ctor=_prefill(True), grad=True),
    _case("mha-prompt13-on-trainmode", "mha", [softmax(13, 13)], "materialized",
          sq=13, use_cache=True, ctor=_prefill(True), train_mode=True),
    _case("mha-step5-off", "mha", [softmax(5, 45)], "materialized", sq=5,
          past=40, use_cache=True, ctor=_prefill(False), pair="mha-step5"),
    _case("mha-step5-on", "mha", [("flash_fwd", 40)], "flash_chunk", sq=5,
          past=40, use_cache=True, ctor=_prefill(True), pair="mha-step5"),
    _case("mha-step1-off", "mha", [DECODE], "decode", sq=1, past=40,
          use_cache=True, ctor=_prefill(False), pair="mha-step1"),
    _case("mha-step1-on", "mha", [DECODE], "decode", sq=1, past=40,
          use_cache=True, ctor=_prefill(True), pair="mha-step1"),
    _case("mha-step1-grad", "mha", [softmax(1, 41)], "materialized", sq=1,
          past=40, use_cache=True, grad=True),
    _case("mha-step1-mask", "mha", [softmax(1, 41)], "materialized", sq=1,
          past=40, use_cache=True, mask="plain"),
    _case("mha-b1-step16-long-on", "mha", [softmax(16, 2080)], "materialized",
          batch=1, past=2064, use_cache=True, ctor=_prefill(True),
          pair="mha-long"),
    _case("mha-b1-step16-long-split", "mha", [("flash_fwd_split", 2064)],
          "flash_chunk_split", batch=1, past=2064, use_cache=True,
          ctor=_prefill("split"), pair="mha-long"),
    _case("mha-b2-step16-long-split", "mha", [softmax(16, 2080)], "materialized",
          batch=2, past=2064, use_cache=True, ctor=_prefill("split")),
    # -- MultiheadAttention, cross-attention (5 queries) ---------------------
    _case("cross-sk16-off", "cross", [softmax(5, 16)], "materialized", sq=5,
          sk_enc=16, ctor=_cross(False)),
    _case("cross-sk16-on", "cross", [FLASH0], "flash_cross", sq=5, sk_enc=16,
          ctor=_cross(True)),
    _case("cross-sk12-on", "cross", [softmax(5, 12)], "materialized", sq=5,
          sk_enc=12, ctor=_cross(True)),
    _case("cross-sk16-on-cached", "cross", [softmax(5, 16)], "materialized",
          sq=5, sk_enc=16, ctor=_cross(True), cross_past=True),
    # -- LlamaAttention ------------------------------------------------------
    _case("llama-train-s16", "llama", [FLASH0, FLASH_BWD], "flash",
          train_mode=True, grad=True, backward=True),
    _case("llama-s12", "llama", [softmax(12, 12)], "unfused", sq=12),
    _case("llama-s16-docs", "llama", [FLASH0], "flash", docs=(10, 6)),
    _case("llama-s12-docs", "llama", [softmax(12, 12)], "unfused", sq=12,
          docs=(7, 5)),
    _case("llama-prompt16-off", "llama", [softmax(16, 16)], "unfused",
          use_cache=True),
    _case("llama-prompt16-off-window8", "llama", [FLASH0], "flash",
          use_cache=True, ctor=dict(sliding_window=8)),
    _case("llama-s12-window8", "llama", [softmax(12, 12)], "unfused", sq=12,
          ctor=dict(sliding_window=8)),
    _case("llama-prompt13-off", "llama", [softmax(13, 13)], "unfused", sq=13,
          use_cache=True, ctor=_prefill(False), pair="llama-prompt13"),
    _case("llama-prompt13-on", "llama", [FLASH0], "flash_prompt", sq=13,
          use_cache=True, ctor=_prefill(True), pair="llama-prompt13"),
    _case("llama-step5-off", "llama", [softmax(5, 45)], "unfused", sq=5,
          past=40, use_cache=True, ctor=_prefill(False), pair="llama-step5"),
    _case("llama-step5-on", "llama", [("flash_fwd", 40)], "flash_chunk", sq=5,
          past=40, use_cache=True, ctor=_prefill(True), pair="llama-step5"),
    _case("llama-step1", "llama", [DECODE], "decode", sq=1, past=40,
          use_cache=True),
    _case("llama-b1-step16-long-on", "llama", [softmax(16, 2080)], "unfused",
          batch=1, past=2064, use_cache=True, ctor=_prefill(True),
          pair="llama-long"),
    _case("llama-b1-step16-long-split", "llama", [("flash_fwd_split", 2064)],
          "flash_chunk_split", batch=1, past=2064, use_cache=True,
          ctor=_prefill("split"), pair="llama-long"),
]

CASE_IDS = [c["id"] for c in CASES]
PAIRS = sorted({c["pair"] for c in CASES if c["pair"]})


def build_layer(case):
    """The layer of a row, freshly initialised from a fixed seed (fp32, CPU):
    rows that differ only in a flag get the same weights."""
    from libai_amd.layers import MultiheadAttention
    from libai_amd.models.llama import LlamaAttention

    torch.manual_seed(7)
    init = torch.nn.init.xavier_normal_
    if case["layer"] == "llama":
        layer = LlamaAttention(LLAMA_HIDDEN, LLAMA_HEADS, LLAMA_MAX_POS, init, init,
                               num_key_value_heads=LLAMA_KV_HEADS, **case["ctor"])
    elif case["layer"] == "cross":
        layer = MultiheadAttention(MHA_HIDDEN, MHA_HEADS, is_cross_attention=True,
                                   **case["ctor"])
    else:
        layer = MultiheadAttention(MHA_HIDDEN, MHA_HEADS, attn_mask_type="causal",
                                   **case["ctor"])
    return layer.train(case["train_mode"])


def key_count(case):
    """Keys the queries of a row attend over, the past included."""
    if case["layer"] == "cross":
        return case["sk_enc"]
    return case["past"] + case["sq"]


def build_mask(case, device):
    """[b, sq, sk] uint8, 1 = masked: right padding that carries ``_kv_len``
    (the second sequence is 5 keys short), or a mask that carries nothing."""
    if case["mask"] is None:
        return None
    b, sq, sk = case["batch"], case["sq"], key_count(case)
    if case["mask"] == "kv_len":
        from libai_amd.models.bert_model import extended_attn_mask

        assert sq == sk
        vis = torch.ones(b, sk, dtype=torch.uint8, device=device)
        vis[1, sk - 5:] = 0
        mask = extended_attn_mask(vis)
        assert mask._kv_len.tolist() == [sk, sk - 5]
        return mask
    mask = torch.zeros(b, sq, sk, dtype=torch.uint8, device=device)
    mask[:, :, 0] = 1  # the first key hidden: no right padding
    return mask


def build_bias(case, device, dtype):
    """``alibi``: the bias of ``build_alibi_bias`` (it carries its slopes);
    ``plain``: a tensor of the same kind of values with no attribute."""
    if case["bias"] is None:
        return None
    sk = key_count(case)
    if case["bias"] == "alibi":
        from libai_amd.layers.position_bias import build_alibi_bias

        return build_alibi_bias(MHA_HEADS, sk, device=device, dtype=dtype)
    gen = torch.Generator().manual_seed(11)
    return torch.randn(MHA_HEADS, case["sq"], sk, generator=gen).to(device, dtype)


def build_docs(case, device):
    """(doc_start, doc_end) int32 [b, s] of the row's packed documents."""
    if case["docs"] is None:
        return None
    starts, ends, at = [], [], 0
    for n in case["docs"]:
        starts += [at] * n
        ends += [at + n] * n
        at += n
    assert at == case["sq"]
    rows = [torch.tensor(x, dtype=torch.int32, device=device)
            .repeat(case["batch"], 1) for x in (starts, ends)]
    return rows[0], rows[1]
