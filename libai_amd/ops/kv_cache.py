"""The e4m3 KV cache of the captured decoders (docs/kernels.md "FP8 KV cache").

Format: ``k8`` / ``v8`` are ``[B, KVH, MAX, HD]`` uint8 tensors holding OCP
e4m3 bytes (``.view(torch.float8_e4m3fn)`` reads them), ``k_scale`` /
``v_scale`` are ``[B, KVH, MAX]`` fp32, one scale per (token, KV head) row:
``scale = amax(row) / 448`` (1.0 for an all-zero row) and
``byte = e4m3(clamp(x / scale, -448, 448))``.
"""

import torch

from ._ext import ext

E4M3_MAX = 448.0
HEAD_DIMS = (64, 128)


def alloc_fp8_cache(b, kvh, max_len, hd, device):
    """-> (c8 [b, kvh, max_len, hd] uint8 zeros, scale [b, kvh, max_len] fp32
    ones): one of the K / V halves of a layer's cache."""
    if hd not in HEAD_DIMS:
        raise ValueError(f"the fp8 KV cache serves head size 64 or 128, got {hd}")
    c8 = torch.zeros(b, kvh, max_len, hd, dtype=torch.uint8, device=device)
    scale = torch.ones(b, kvh, max_len, dtype=torch.float32, device=device)
    return c8, scale


def quantize_rows(src, c8, scale):
    """Quantizes ``src`` [B, KVH, L, HD] bf16 (strided views with a contiguous
    last dim are taken as they are) into rows [0, L) of ``c8`` and ``scale``."""
    if src.dim() != 4 or c8.dim() != 4:
        raise ValueError("src must be [B, KVH, L, HD] and c8 [B, KVH, MAX, HD]")
    if (src.shape[0], src.shape[1], src.shape[3]) != (c8.shape[0], c8.shape[1],
                                                      c8.shape[3]):
        raise ValueError(f"src {tuple(src.shape)} does not fit the cache "
                         f"{tuple(c8.shape)}")
    if src.shape[2] > c8.shape[2]:
        raise ValueError(f"{src.shape[2]} rows exceed the cache capacity "
                         f"{c8.shape[2]}")
    if tuple(scale.shape) != tuple(c8.shape[:3]):
        raise ValueError(f"scale must be {tuple(c8.shape[:3])}, got "
                         f"{tuple(scale.shape)}")
    if src.stride(3) != 1:
        src = src.contiguous()
    ext().kv_quantize_rows(src, c8, scale)


def accept_greedy(draft, target):
    """Greedy speculative acceptance, on the device with no host read.

    ``draft`` [B, K] are the proposed tokens, ``target`` [B, K + 1] the model's
    argmax after the last accepted token and after each draft token.  ->
    ``(n [B], next_tok [B, 1])``: n is the length of the leading run with
    ``draft[:, i] == target[:, i]``, next_tok the model's own token behind it,
    ``target[b, n[b]]``."""
    if draft.dim() != 2 or tuple(target.shape) != (draft.shape[0], draft.shape[1] + 1):
        raise ValueError(f"draft [B, K] and target [B, K + 1], got "
                         f"{tuple(draft.shape)} and {tuple(target.shape)}")
    n = (draft == target[:, :-1]).long().cumprod(dim=1).sum(dim=1)
    return n, target.gather(1, n[:, None])


def dequantize(c8, scale):
    """fp32 values of a cache half, plain torch (tests and debugging)."""
    return c8.view(torch.float8_e4m3fn).to(torch.float32) * scale.unsqueeze(-1)
