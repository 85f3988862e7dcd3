"""Document boundaries of packed samples (host side, no kernel).

A packed sample is several documents concatenated into one row.  The flash
kernels and the Llama family keep attention and RoPE inside each document
when they get, per token i of the row,

  doc_start[i]     index of the first token of the document that holds i
  doc_end[i]       one past that document's last token
  position_ids[i]  i - doc_start[i]

(Megatron's ``reset_attention_mask`` / ``reset_position_ids``; flash-attn's
``cu_seqlens`` carry the same information.)  All three are int32.
"""

import numpy as np
import torch

__all__ = ["doc_bounds_from_lengths", "doc_bounds_from_doc_ids"]


def doc_bounds_from_lengths(lengths, seq_length):
    """lengths: the documents' token counts, in row order ->
    (doc_start, doc_end, position_ids), int32 [seq_length] each.

    The lengths may cover less than the row: every token of the uncovered tail
    (padding) becomes a one-token document.  Raises ValueError on a length
    < 1, on lengths that overrun the row and on a row of no tokens."""
    seq_length = int(seq_length)
    if seq_length < 1:
        raise ValueError(f"seq_length must be >= 1, got {seq_length}")
    lengths = np.asarray(lengths)
    if lengths.ndim != 1:
        raise ValueError(f"lengths must be a flat sequence, got shape {lengths.shape}")
    if lengths.size and not np.issubdtype(lengths.dtype, np.integer):
        raise ValueError(f"lengths must be integers, got {lengths.dtype}")
    lengths = lengths.astype(np.int64)
    if (lengths < 1).any():
        raise ValueError(f"every document needs at least one token, got {lengths.tolist()}")
    covered = int(lengths.sum())
    if covered > seq_length:
        raise ValueError(
            f"documents of {covered} tokens do not fit a row of {seq_length}")
    lengths = np.concatenate([lengths, np.ones(seq_length - covered, dtype=np.int64)])
    ends = np.cumsum(lengths)
    doc_start = np.repeat(ends - lengths, lengths)
    doc_end = np.repeat(ends, lengths)
    pos = np.arange(seq_length, dtype=np.int64) - doc_start
    return tuple(torch.from_numpy(a.astype(np.int32)) for a in (doc_start, doc_end, pos))


def doc_bounds_from_doc_ids(doc_ids):
    """doc_ids: integer [..., S], one id per token; a new document starts
    wherever the id changes along the last dimension ->
    (doc_start, doc_end, position_ids), int32 [..., S] each, on doc_ids'
    device.  Raises ValueError on a non-integer or empty input."""
    doc_ids = torch.as_tensor(doc_ids)
    if doc_ids.dim() < 1 or doc_ids.shape[-1] < 1:
        raise ValueError(f"doc_ids must be [..., S] with S >= 1, got {tuple(doc_ids.shape)}")
    if doc_ids.is_floating_point() or doc_ids.is_complex() or doc_ids.dtype == torch.bool:
        raise ValueError(f"doc_ids must be integers, got {doc_ids.dtype}")
    s = doc_ids.shape[-1]
    pos = torch.arange(s, device=doc_ids.device).expand(doc_ids.shape)
    first = torch.ones_like(doc_ids, dtype=torch.bool)
    first[..., 1:] = doc_ids[..., 1:] != doc_ids[..., :-1]
    # start: the latest document head at or before i (running maximum)
    doc_start = torch.where(first, pos, torch.zeros_like(pos)).cummax(dim=-1).values
    # end: the earliest document head after i (running minimum from the right)
    nxt = torch.full_like(pos, s)
    nxt[..., :-1] = torch.where(first[..., 1:], pos[..., 1:], nxt[..., 1:])
    doc_end = nxt.flip(-1).cummin(dim=-1).values.flip(-1)
    return (doc_start.to(torch.int32), doc_end.to(torch.int32),
            (pos - doc_start).to(torch.int32))
