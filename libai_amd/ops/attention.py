"""Fused flash-style attention (bf16, MFMA) with recompute backward.

Forward: one HIP kernel (libai_amd/csrc/kernels/flash_attn.hip) — the S x S
score matrix never touches HBM; O and the per-row logsumexp are saved.

Padding masks: BERT/RoBERTa-style right-padded batches are expressed as a
per-sequence valid key length (int32 [B]); the kernels mask kv >= kv_len[b]
in-register, replacing the reference's additive -10000 [b, s, s] mask
(reference libai/layers/attention.py:221-226) without materializing scores.

ALiBi (BLOOM): an optional fp32 ``alibi_slopes`` [H] (one per query head of
the call) makes the kernels add slope[h] * (kv - q) to every pre-softmax
score in-register — no bias tensor in HBM and, the slopes being constants, no
bias gradient.  (kv - q) is row-shift-equivalent to BLOOM's slope * kv.

Sliding window (Mistral): an optional integer ``window`` W >= 1 restricts
causal attention to the last W keys, the query's own included (query i sees
key j iff j <= i and i - j < W, HF's ``q_idx - kv_idx < sliding_window``).
The kernels mask in-register and skip every tile below the band.  ``None`` or
0 means off; a window covering the whole sequence is normalized to off.

Relative-position bias (T5/MT5): an optional fp32 ``rel_bias`` [H, Sq+Sk-1]
(one row per query head) makes the kernels add rel_bias[h, kv - q + Sq - 1]
to every pre-softmax score in-register.  The bias is Toeplitz, so the
[H, Sq, Sk] tensor never exists; the table is learned, so the backward also
returns its gradient (dS without the scale, summed along diagonals with fp32
atomics: summation-order dependent in its last bits, like the embedding
backward).  Not combinable with ``alibi_slopes`` or ``window``.

Packed documents (Megatron ``reset_attention_mask``, flash-attn varlen): an
optional ``doc_bounds`` pair ``(doc_start, doc_end)`` of int32 [B, S] tensors
keeps causal attention inside the query's own document: query i sees key j
iff doc_start[b, i] <= j <= i.  doc_start[b, i] is the first token of the
document holding token i, doc_end[b, i] one past its last
(``libai_amd.data.packing`` builds both).  The kernels mask in-register and
walk only the tiles on the block diagonal.  Composes with GQA, dropout and
``kv_len``; not combinable with ``alibi_slopes``, ``window``, ``rel_bias`` or
``causal=False``, and needs Sq == Sk.

Query offset (a chunk behind cached keys): ``flash_attention(...,
q_offset=n)`` places query row i at key position n + i, so the causal mask,
the window and the ALiBi distance are taken there; ``q_offset = Sk - Sq`` is
the bottom-right alignment a ``cat([past, new])`` cache needs.  Inference
only (no backward, no dropout); plain, ALiBi and window variants; the key
count may be ragged.  ``q_offset = 0`` is the call it always was, top-left
alignment for Sq != Sk included.

Cross-attention (T5/MT5 decoder): ``flash_attention_kv`` takes the query
projection and the packed [B, Sk, H, 2, D] key/value projection, non-causal,
Sq != Sk; its backward writes dK and dV into one packed allocation.

Replaces the reference's K2-K5 chain (reference
libai/layers/attention.py:211-253).
"""

from typing import NamedTuple, Optional

import torch

from ._ext import draw_seed, ext

__all__ = ["flash_attention", "flash_attention_qkv", "flash_attention_kv",
           "flash_attention_available", "flash_prefill_available",
           "flash_cross_available", "flash_chunk_pays", "mask_kv_len", "bias_alibi_slopes",
           "bias_rel_table"]


def mask_kv_len(pad_mask):
    """The per-sequence valid-length tensor attached to a padding mask by
    ``extended_attn_mask`` when the mask is pure right-padding, else None."""
    return getattr(pad_mask, "_kv_len", None) if pad_mask is not None else None


def bias_alibi_slopes(position_bias):
    """The fp32 per-head slopes attached to a bias by ``build_alibi_bias``
    (the bias is then exactly ALiBi and the kernels can fuse it), else None."""
    if position_bias is None:
        return None
    return getattr(position_bias, "_alibi_slopes", None)


def bias_rel_table(position_bias):
    """The fp32 [nh, sq + sk - 1] diagonal table attached to a bias by
    ``T5RelativePositionBias`` (the bias is then exactly Toeplitz and the
    kernels can fuse it, gradient included), else None."""
    if position_bias is None:
        return None
    return getattr(position_bias, "_rel_bias_table", None)


class _Variant(NamedTuple):
    """The kernel variant arguments, in the order ``_C.flash_fwd`` and
    ``_C.flash_bwd`` take them after ``kv_len``.  At most one variant is on."""

    alibi_slopes: Optional[torch.Tensor] = None  # constant: no grad flows to it
    window: int = 0                              # 0 = off
    rel_bias: Optional[torch.Tensor] = None      # learned: the one with a grad
    doc_start: Optional[torch.Tensor] = None     # int32: no grad flows to them
    doc_end: Optional[torch.Tensor] = None


def _variant_args(n_keys, causal=True, alibi_slopes=None, window=None, rel_bias=None,
                  doc_bounds=None):
    """Checks the variant arguments against each other and normalizes them: a
    window of None or 0, or one that covers all n_keys keys (it masks nothing
    and runs the windowless instantiation), is off."""
    windowed = window is not None and window != 0
    if doc_bounds is not None:
        if not causal:
            raise ValueError("doc_bounds requires causal attention")
        if alibi_slopes is not None:
            raise ValueError("doc_bounds cannot be combined with alibi_slopes")
        if windowed:
            raise ValueError("doc_bounds cannot be combined with a sliding window")
        if rel_bias is not None:
            raise ValueError("doc_bounds cannot be combined with rel_bias")
        if doc_bounds[0] is None or doc_bounds[1] is None:
            raise ValueError("doc_bounds needs both doc_start and doc_end")
    if rel_bias is not None:
        if alibi_slopes is not None:
            raise ValueError("rel_bias cannot be combined with alibi_slopes")
        if windowed:
            raise ValueError("rel_bias cannot be combined with a sliding window")
    if windowed:
        window = int(window)
        if window < 0:
            raise ValueError(f"window must be >= 1 (or None/0 for off), got {window}")
        if not causal:
            raise ValueError("a sliding window requires causal attention")
        if alibi_slopes is not None:
            raise ValueError("a sliding window cannot be combined with alibi_slopes")
    doc_start, doc_end = doc_bounds if doc_bounds is not None else (None, None)
    return _Variant(alibi_slopes, window if windowed and window < n_keys else 0,
                    rel_bias, doc_start, doc_end)


def _save_variant(ctx, variant, *tensors):
    """Saves the forward's tensors, the table included when there is one."""
    has_rel_bias = variant.rel_bias is not None
    ctx.save_for_backward(*tensors, *([variant.rel_bias] if has_rel_bias else []))
    ctx.variant = variant._replace(rel_bias=None)  # the table lives in saved_tensors
    ctx.has_rel_bias = has_rel_bias


def _saved_variant(ctx):
    """-> (the tensors given to _save_variant, the variant as it was saved)."""
    saved = ctx.saved_tensors
    if not ctx.has_rel_bias:
        return saved, ctx.variant
    return saved[:-1], ctx.variant._replace(rel_bias=saved[-1])


def _variant_grads(ctx, first, grads):
    """The backward's return values for the variant inputs, which start at
    input `first`: the table's gradient (flash_bwd appends it to dq, dk, dv
    when there is a table) where it is wanted, None everywhere else."""
    at = first + _Variant._fields.index("rel_bias")
    d_rel = grads[3] if ctx.has_rel_bias and ctx.needs_input_grad[at] else None
    return tuple(_Variant(window=None, rel_bias=d_rel))


def flash_attention_available(head_dim, dtype, device, sq, sk, pad_mask):
    return (
        device.type == "cuda"
        and dtype == torch.bfloat16
        and head_dim in (64, 128)
        and (pad_mask is None or mask_kv_len(pad_mask) is not None)
        and sk % 8 == 0
        and sq == sk  # training self-attention (no KV-cache decode)
    )


def flash_prefill_available(head_dim, dtype, device, sq, sk):
    """The inference forward over cached keys (``flash_attention`` with
    ``q_offset = sk - sq``, or the square prompt pass): any key count, ragged
    included; no gradients."""
    return (
        device.type == "cuda"
        and dtype == torch.bfloat16
        and head_dim in (64, 128)
        and 1 <= sq <= sk
        and not torch.is_grad_enabled()
    )


# The chunk route runs one workgroup per 128 queries and head, and each walks
# all the keys serially.  profiles/flash_prefill_cross.md, section 2, batch 1
# and 32 heads: with 32 workgroups (chunks up to 128 tokens) it measured
# faster than the materialized route on 256 to 1024 cached keys, 1.1-1.5x
# slower on 2048 and 1.5-2.2x slower on 4096; with 128 workgroups (a 512-token
# chunk) 1.04-1.23x slower on 4096.  Long caches under few workgroups keep the
# materialized route; fuller grids were not measured.
FLASH_CHUNK_LONG_CACHE = 2048      # keys
FLASH_CHUNK_FEW_WORKGROUPS = 128   # batch * heads * ceil(sq / 128)


def flash_chunk_pays(batch, heads, sq, sk):
    """Whether a chunk of sq queries behind a cache (sk keys in all) should
    take the flash forward: not a few workgroups walking a long cache."""
    workgroups = batch * heads * -(-sq // 128)
    return sk < FLASH_CHUNK_LONG_CACHE or workgroups > FLASH_CHUNK_FEW_WORKGROUPS


def flash_cross_available(head_dim, dtype, device, sq, sk, pad_mask):
    """Non-causal attention of sq queries over sk other keys
    (``flash_attention_kv``), forward and backward."""
    return (
        device.type == "cuda"
        and dtype == torch.bfloat16
        and head_dim in (64, 128)
        and (pad_mask is None or mask_kv_len(pad_mask) is not None)
        and sk % 8 == 0
        and sq >= 1
    )


class _FlashAttnQKVFn(torch.autograd.Function):
    """Packed-qkv variant: takes the fused [B, S, H, 3, D] projection buffer
    directly.  The backward writes dQ/dK/dV straight into one packed dqkv
    allocation (the HIP kernels take strides), so autograd never materializes
    three view-grads and scatter-adds them into a zeroed buffer -- that glue
    measured ~5 ms/step on GPT-2 345M (three 50M-element passes per layer).
    """

    @staticmethod
    def forward(ctx, qkv5, scale, p_drop, causal, kv_len, *variant):
        q = qkv5[..., 0, :]
        k = qkv5[..., 1, :]
        v = qkv5[..., 2, :]
        seed = draw_seed() if p_drop > 0 else 0
        o, lse = ext().flash_fwd(q, k, v, scale, p_drop, seed, causal, kv_len,
                                 *variant)
        _save_variant(ctx, _Variant(*variant), qkv5, o, lse)
        ctx.kv_len = kv_len
        ctx.meta = (scale, p_drop, seed, causal)
        return o

    @staticmethod
    def backward(ctx, do):
        (qkv5, o, lse), variant = _saved_variant(ctx)
        scale, p_drop, seed, causal = ctx.meta
        dqkv = torch.empty_like(qkv5)
        grads = ext().flash_bwd(
            qkv5[..., 0, :], qkv5[..., 1, :], qkv5[..., 2, :], o, do.contiguous(),
            lse, scale, p_drop, seed, causal, dqkv, ctx.kv_len, *variant,
        )
        # inputs: qkv5, scale, p_drop, causal, kv_len, then the variant
        return (dqkv, None, None, None, None) + _variant_grads(ctx, 5, grads)


def flash_attention_qkv(qkv5, scale, p_drop=0.0, causal=True, training=True,
                        kv_len=None, alibi_slopes=None, window=None,
                        rel_bias=None, doc_bounds=None):
    """qkv5: packed [B, S, H, 3, D] bf16 -> O [B, S, H, D] (zero-copy in/out).

    kv_len: optional int32 [B] — keys at/after kv_len[b] are masked out.
    alibi_slopes: optional fp32 [H] — adds slope[h] * (kv - q) to the scores.
    window: optional int W — causal sliding window over the last W keys.
    rel_bias: optional fp32 [H, 2S-1] — adds rel_bias[h, kv - q + S - 1] to the
    scores; differentiable (not combinable with alibi_slopes or window).
    doc_bounds: optional (doc_start, doc_end), int32 [B, S] each — packed
    documents: query i sees key j iff doc_start[b, i] <= j <= i."""
    variant = _variant_args(qkv5.shape[1], causal, alibi_slopes, window, rel_bias,
                            doc_bounds)
    return _FlashAttnQKVFn.apply(qkv5, scale, p_drop if training else 0.0, causal,
                                 kv_len, *variant)


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, p_drop, causal, kv_len, *variant):
        # q, k, v: [B, S, H, D] (may be strided views of the fused qkv buffer)
        seed = draw_seed() if p_drop > 0 else 0
        o, lse = ext().flash_fwd(q, k, v, scale, p_drop, seed, causal, kv_len,
                                 *variant)
        _save_variant(ctx, _Variant(*variant), q, k, v, o, lse)
        ctx.kv_len = kv_len
        ctx.meta = (scale, p_drop, seed, causal)
        return o

    @staticmethod
    def backward(ctx, do):
        (q, k, v, o, lse), variant = _saved_variant(ctx)
        scale, p_drop, seed, causal = ctx.meta
        grads = ext().flash_bwd(
            q, k, v, o, do.contiguous(), lse, scale, p_drop, seed, causal, None,
            ctx.kv_len, *variant,
        )
        # inputs: q, k, v, scale, p_drop, causal, kv_len, then the variant
        dq, dk, dv = grads[:3]
        return (dq, dk, dv, None, None, None, None) + _variant_grads(ctx, 7, grads)


class _FlashAttnKVFn(torch.autograd.Function):
    """Cross-attention on the packed key/value projection: q [B, Sq, H, D] and
    kv5 [B, Sk, H, 2, D], non-causal.  The backward writes dK/dV straight into
    one packed dkv allocation, as _FlashAttnQKVFn does with dqkv."""

    @staticmethod
    def forward(ctx, q, kv5, scale, p_drop, kv_len):
        seed = draw_seed() if p_drop > 0 else 0
        o, lse = ext().flash_fwd(q, kv5[..., 0, :], kv5[..., 1, :], scale, p_drop,
                                 seed, False, kv_len)
        ctx.save_for_backward(q, kv5, o, lse)
        ctx.kv_len = kv_len
        ctx.meta = (scale, p_drop, seed)
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv5, o, lse = ctx.saved_tensors
        scale, p_drop, seed = ctx.meta
        dkv = torch.empty_like(kv5)
        dq = ext().flash_bwd(
            q, kv5[..., 0, :], kv5[..., 1, :], o, do.contiguous(), lse, scale,
            p_drop, seed, False, None, ctx.kv_len, dkv=dkv,
        )[0]
        return dq, dkv, None, None, None


def flash_attention_kv(q, kv5, scale, p_drop=0.0, training=True, kv_len=None):
    """q: [B, Sq, H, D], kv5: packed [B, Sk, H, 2, D] bf16 -> O [B, Sq, H, D]
    (zero-copy in/out).  Non-causal: every query sees every key below
    kv_len[b] (optional int32 [B]).  Sq and Sk are independent."""
    if kv5.dim() != 5 or kv5.shape[3] != 2:
        raise ValueError(f"kv5 must be [B, Sk, H, 2, D], got {tuple(kv5.shape)}")
    return _FlashAttnKVFn.apply(q, kv5, scale, p_drop if training else 0.0, kv_len)


def _check_q_offset(q_offset, sq, sk, causal, p_drop, rel_bias, doc_bounds):
    """The rules of a non-zero query offset, before anything reaches the
    extension."""
    if q_offset < 0:
        raise ValueError(f"q_offset must be >= 0, got {q_offset}")
    if q_offset == 0:
        return
    if not causal:
        raise ValueError("q_offset requires causal attention")
    if p_drop > 0:
        raise ValueError("q_offset cannot be combined with dropout")
    if rel_bias is not None:
        raise ValueError("q_offset cannot be combined with rel_bias")
    if doc_bounds is not None:
        raise ValueError("q_offset cannot be combined with doc_bounds")
    if q_offset + sq > sk:
        raise ValueError(f"q_offset + Sq must not exceed Sk "
                         f"({q_offset} + {sq} > {sk})")


def flash_attention(q, k, v, scale, p_drop=0.0, causal=True, training=True,
                    kv_len=None, alibi_slopes=None, window=None, rel_bias=None,
                    doc_bounds=None, q_offset=0):
    """q, k, v: [B, S, H, D] bf16 -> O [B, S, H, D].

    alibi_slopes: optional fp32 [H] (query heads) — fused ALiBi bias.
    window: optional int W — causal sliding window: query i sees the keys
    j <= i with i - j < W (not combinable with alibi_slopes or causal=False).
    rel_bias: optional fp32 [H, Sq+Sk-1] (query heads) — fused Toeplitz bias
    rel_bias[h, kv - q + Sq - 1]; differentiable (its gradient is summed over
    the batch), not combinable with alibi_slopes or window.
    doc_bounds: optional (doc_start, doc_end), int32 [B, S] each — packed
    documents: causal attention that stays inside the query's own document
    (needs Sq == Sk; not combinable with alibi_slopes, window, rel_bias or
    causal=False).
    q_offset: optional int n > 0 — query row i sits at key position n + i (a
    chunk behind n cached keys; n = Sk - Sq for a cat([past, new]) cache).
    Inference only: causal, no dropout, no gradients, plain / alibi_slopes /
    window; Sk may be ragged.  0 = off."""
    q_offset = int(q_offset)
    p_drop = p_drop if training else 0.0
    _check_q_offset(q_offset, q.shape[1], k.shape[1], causal, p_drop, rel_bias,
                    doc_bounds)
    variant = _variant_args(k.shape[1], causal, alibi_slopes, window, rel_bias,
                            doc_bounds)
    if q_offset > 0:
        if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad
                                        or v.requires_grad):
            raise ValueError("q_offset is an inference path: it has no backward")
        return ext().flash_fwd(q, k, v, scale, 0.0, 0, True, kv_len, *variant,
                               q_offset)[0]
    return _FlashAttnFn.apply(q, k, v, scale, p_drop, causal, kv_len, *variant)


def decode_attention_available(q, head_dim):
    """Fused single-query decode path (K16): inference, bf16, D in {64,128}."""
    return (
        q.device.type == "cuda"
        and q.dtype == torch.bfloat16
        and head_dim in (64, 128)
        and not torch.is_grad_enabled()
        and q.shape[-2] == 1
    )


def flash_decode_attn(q, k, v, scale, kv_len=None, alibi_slopes=None,
                      window=None):
    """q [B, H, 1, D], k/v [B, Hkv, Skv, D] (KV-cache layout) -> [B, H, 1, D].

    One fused kernel: online-softmax q.K^T -> .V, GQA head mapping in-kernel
    (replaces the decode bmm+softmax+bmm chain; reference capability
    flow._C.fused_multi_head_attention_inference_v2).

    alibi_slopes: optional fp32 [H] — adds slope[h] * (key - qpos) with the
    query at the last valid key, qpos = kv_len[b] - 1 (Skv - 1 if no kv_len).
    window: optional int W — only the last W valid keys are visible (and read):
    [max(0, kv_len[b] - W), kv_len[b])."""
    variant = _variant_args(k.shape[2], True, alibi_slopes, window)
    return ext().flash_decode(q, k, v, scale, kv_len, variant.alibi_slopes,
                              variant.window)
