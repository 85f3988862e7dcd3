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

Replaces the reference's K2-K5 chain (reference
libai/layers/attention.py:211-253).
"""

import torch

from ._ext import draw_seed, ext

__all__ = ["flash_attention", "flash_attention_qkv", "flash_attention_available",
           "mask_kv_len", "bias_alibi_slopes"]


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


def flash_attention_available(head_dim, dtype, device, sq, sk, pad_mask):
    return (
        device.type == "cuda"
        and dtype == torch.bfloat16
        and head_dim in (64, 128)
        and (pad_mask is None or mask_kv_len(pad_mask) is not None)
        and sk % 8 == 0
        and sq == sk  # training self-attention (no KV-cache decode)
    )


class _FlashAttnQKVFn(torch.autograd.Function):
    """Packed-qkv variant: takes the fused [B, S, H, 3, D] projection buffer
    directly.  The backward writes dQ/dK/dV straight into one packed dqkv
    allocation (the HIP kernels take strides), so autograd never materializes
    three view-grads and scatter-adds them into a zeroed buffer -- that glue
    measured ~5 ms/step on GPT-2 345M (three 50M-element passes per layer).
    """

    @staticmethod
    def forward(ctx, qkv5, scale, p_drop, causal, kv_len, alibi_slopes=None):
        q = qkv5[..., 0, :]
        k = qkv5[..., 1, :]
        v = qkv5[..., 2, :]
        seed = draw_seed() if p_drop > 0 else 0
        o, lse = ext().flash_fwd(q, k, v, scale, p_drop, seed, causal, kv_len,
                                 alibi_slopes)
        ctx.save_for_backward(qkv5, o, lse)
        ctx.kv_len = kv_len
        ctx.alibi_slopes = alibi_slopes  # constant: no grad flows to it
        ctx.meta = (scale, p_drop, seed, causal)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv5, o, lse = ctx.saved_tensors
        scale, p_drop, seed, causal = ctx.meta
        dqkv = torch.empty_like(qkv5)
        ext().flash_bwd(
            qkv5[..., 0, :], qkv5[..., 1, :], qkv5[..., 2, :], o, do.contiguous(),
            lse, scale, p_drop, seed, causal, dqkv, ctx.kv_len,
            ctx.alibi_slopes,
        )
        return dqkv, None, None, None, None, None


def flash_attention_qkv(qkv5, scale, p_drop=0.0, causal=True, training=True,
                        kv_len=None, alibi_slopes=None):
    """qkv5: packed [B, S, H, 3, D] bf16 -> O [B, S, H, D] (zero-copy in/out).

    kv_len: optional int32 [B] — keys at/after kv_len[b] are masked out.
    alibi_slopes: optional fp32 [H] — adds slope[h] * (kv - q) to the scores."""
    return _FlashAttnQKVFn.apply(qkv5, scale, p_drop if training else 0.0, causal,
                                 kv_len, alibi_slopes)


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, p_drop, causal, kv_len, alibi_slopes=None):
        # q, k, v: [B, S, H, D] (may be strided views of the fused qkv buffer)
        seed = draw_seed() if p_drop > 0 else 0
        o, lse = ext().flash_fwd(q, k, v, scale, p_drop, seed, causal, kv_len,
                                 alibi_slopes)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.kv_len = kv_len
        ctx.alibi_slopes = alibi_slopes
        ctx.meta = (scale, p_drop, seed, causal)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        scale, p_drop, seed, causal = ctx.meta
        dq, dk, dv = ext().flash_bwd(
            q, k, v, o, do.contiguous(), lse, scale, p_drop, seed, causal, None,
            ctx.kv_len, ctx.alibi_slopes,
        )
        return dq, dk, dv, None, None, None, None, None


def flash_attention(q, k, v, scale, p_drop=0.0, causal=True, training=True,
                    kv_len=None, alibi_slopes=None):
    """q, k, v: [B, S, H, D] bf16 -> O [B, S, H, D].

    alibi_slopes: optional fp32 [H] (query heads) — fused ALiBi bias."""
    return _FlashAttnFn.apply(q, k, v, scale, p_drop if training else 0.0, causal,
                              kv_len, alibi_slopes)


def decode_attention_available(q, head_dim):
    """Fused single-query decode path (K16): inference, bf16, D in {64,128}."""
    return (
        q.device.type == "cuda"
        and q.dtype == torch.bfloat16
        and head_dim in (64, 128)
        and not torch.is_grad_enabled()
        and q.shape[-2] == 1
    )


def flash_decode_attn(q, k, v, scale, kv_len=None, alibi_slopes=None):
    """q [B, H, 1, D], k/v [B, Hkv, Skv, D] (KV-cache layout) -> [B, H, 1, D].

    One fused kernel: online-softmax q.K^T -> .V, GQA head mapping in-kernel
    (replaces the decode bmm+softmax+bmm chain; reference capability
    flow._C.fused_multi_head_attention_inference_v2).

    alibi_slopes: optional fp32 [H] — adds slope[h] * (key - qpos) with the
    query at the last valid key, qpos = kv_len[b] - 1 (Skv - 1 if no kv_len)."""
    return ext().flash_decode(q, k, v, scale, kv_len, alibi_slopes)
