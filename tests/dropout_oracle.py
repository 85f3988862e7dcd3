"""Dropout-mask oracle for the HIP kernels, written from the definitions in
csrc/kernels/common.h (rnd_hash2, rnd_hash, drop_threshold_u8) and
csrc/kernels/flash_attn.hip (drop_hash4), in numpy uint64 arithmetic reduced
mod 2^32.  It shares no code with the kernels, runs on the CPU and is the
reference the GPU dropout tests compare against.

One 32-bit hash yields four keep decisions: byte `i & 3` of the hash keyed on
`i >> 2` is compared `>= thr8`, with `thr8 = min(255, int(p * 256 + 0.5))`.
The keep rate is therefore (256 - thr8) / 256, not 1 - p, while kept values
are scaled by 1 / (1 - p).
"""

import numpy as np
import torch

_M32 = np.uint64(0xFFFFFFFF)


def drop_threshold_u8(p):
    """Byte threshold of the kernels: p quantised to 1/256, in fp32."""
    t = np.float32(p) * np.float32(256.0) + np.float32(0.5)
    return 255 if t >= np.float32(255.0) else int(t)


def keep_rate(p):
    """Expected fraction of kept elements: (256 - thr8) / 256."""
    return (256 - drop_threshold_u8(p)) / 256.0


def keep_scale(p):
    """The kernels' fp32 1 / (1 - p) (1 when p == 0)."""
    if p <= 0:
        return np.float32(1.0)
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def rnd_hash2(seed, lo, hi):
    """common.h rnd_hash2: lo/hi are uint64 arrays holding 32-bit values."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = np.uint64((seed & 0xFFFFFFFF) ^ (seed >> 32))
    lo = np.asarray(lo, dtype=np.uint64) & _M32
    hi = np.asarray(hi, dtype=np.uint64) & _M32
    h = s ^ ((lo * np.uint64(0x9E3779B9)) & _M32) ^ ((hi * np.uint64(0x85EBCA6B)) & _M32)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & _M32
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & _M32
    h = h ^ (h >> np.uint64(16))
    return h


def _bytes_keep(h4, n_last, thr8):
    """[..., n4] hashes -> bool [..., n_last]: byte j of hash i decides 4*i+j."""
    shifts = (np.arange(4, dtype=np.uint64) * np.uint64(8))
    b = (h4[..., None] >> shifts) & np.uint64(0xFF)
    keep = b >= np.uint64(thr8)
    return keep.reshape(*h4.shape[:-1], -1)[..., :n_last]


def attn_keep_mask(seed, BH, Sq, Sk, p):
    """Attention dropout mask, bool [BH, Sq, Sk] (True = kept): the hash is
    rnd_hash2(seed, lo = q * (Sk >> 2) + (kv >> 2), hi = bh), byte kv & 3."""
    sk4 = Sk >> 2
    n4 = (Sk + 3) // 4
    q = np.arange(Sq, dtype=np.uint64)[None, :, None]
    kv4 = np.arange(n4, dtype=np.uint64)[None, None, :]
    bh = np.arange(BH, dtype=np.uint64)[:, None, None]
    lo = (q * np.uint64(sk4) + kv4) & _M32
    h = rnd_hash2(seed, np.broadcast_to(lo, (BH, Sq, n4)),
                  np.broadcast_to(bh, (BH, Sq, n4)))
    return torch.from_numpy(_bytes_keep(h, Sk, drop_threshold_u8(p)))


def elem_keep_mask(seed, n, p):
    """Elementwise dropout mask of the bias+dropout+residual kernel, bool [n]:
    rnd_hash(seed, idx = elem // 4), byte elem % 4 (the same for bf16 and
    fp32: (i * (V / 4) + q) is elem // 4 for both vector widths)."""
    n4 = (n + 3) // 4
    idx = np.arange(n4, dtype=np.uint64)
    h = rnd_hash2(seed, idx & _M32, idx >> np.uint64(32))
    return torch.from_numpy(_bytes_keep(h, n, drop_threshold_u8(p)))


def ref_attention_probs(q, k, scale, causal, kv_len=None, alibi_slopes=None,
                        window=0):
    """fp32 softmax probabilities [B, H, Sq, Sk] for [B, S, H, D] q and
    [B, S, Hkv, D] k.  Query i sees key j iff j < kv_len[b], j <= i + Sk - Sq
    when causal, and i - j < window when window > 0; ALiBi adds
    slope[h] * (j - i).  Rows without a visible key give zeros."""
    group = q.shape[2] // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    sq, sk = s.shape[-2], s.shape[-1]
    i = torch.arange(sq, device=q.device)[:, None]
    j = torch.arange(sk, device=q.device)[None, :]
    if alibi_slopes is not None:
        rel = (j - i).float()
        s = s + alibi_slopes.float()[None, :, None, None] * rel[None, None]
    visible = torch.ones(sq, sk, dtype=torch.bool, device=q.device)
    if causal:
        visible = visible & (j <= i + (sk - sq))
    if window:
        visible = visible & (i - j < window)
    visible = visible[None, None]
    if kv_len is not None:
        visible = visible & (j[None, None] < kv_len[:, None, None, None])
    s = s.masked_fill(~visible, float("-inf"))
    has_key = visible.any(-1, keepdim=True)
    s = torch.where(has_key, s, torch.zeros_like(s))  # keep empty rows finite
    return torch.softmax(s, dim=-1) * has_key


def ref_attention_masked(q, k, v, scale, keep, keep_scale, causal, kv_len=None,
                         alibi_slopes=None, window=0):
    """fp32, differentiable O = (softmax(S) * keep * keep_scale) @ V on
    [B, S, H, D] / [B, S, Hkv, D] inputs (GQA by repeat_interleave); keep is
    [B * H, Sq, Sk] or [B, H, Sq, Sk].  Returns [B, Sq, H, D]."""
    group = q.shape[2] // k.shape[2]
    p = ref_attention_probs(q, k, scale, causal, kv_len=kv_len,
                            alibi_slopes=alibi_slopes, window=window)
    keep = keep.to(device=p.device, dtype=torch.float32).reshape(p.shape)
    pd = p * keep * float(keep_scale)
    vh = v.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    return torch.matmul(pd, vh).permute(0, 2, 1, 3)
