"""Mixture-of-Experts routing, dispatch and combine (csrc/kernels/moe.hip).

Three ops around the expert GEMMs of ``layers/moe.py``:

  gates, idx, counts, psum, plan = moe_route(logits, k)
  xk = moe_permute(x, plan)             # [n*k, H], grouped by expert
  y  = moe_combine(yk, gates, plan, residual=None)

``plan`` is the stable counting sort of the n*k copies (copy f = i*k + j) by
expert: the order ``torch.argsort(idx.reshape(-1), stable=True)`` gives.

CUDA tensors run the HIP kernels (fp32 routing, fp32 gate-weighted sum with
one rounding).  CPU tensors run the torch composition ``MoELayer`` uses, which
is also the numerics reference of the GPU tests.
"""

from collections import namedtuple

import torch

from ._ext import ext, use_hip

__all__ = ["MoEPlan", "moe_route", "moe_permute", "moe_combine",
           "moe_fused_available"]

MAX_EXPERTS = 256
MAX_TOP_K = 8

# slot[f]: row of copy f in the expert-sorted layout; row_of_slot: its inverse;
# expert_offsets[e] .. [e+1]: the rows of expert e
MoEPlan = namedtuple("MoEPlan", ["slot", "row_of_slot", "expert_offsets", "k"])


def _route_problem(n, E, k, dtype=torch.float32):
    if dtype != torch.float32:
        return f"router logits must be fp32, got {dtype}"
    if not 1 <= E <= MAX_EXPERTS:
        return f"1 <= num_experts <= {MAX_EXPERTS}, got {E}"
    if not 1 <= k <= min(E, MAX_TOP_K):
        return f"1 <= top_k <= min(num_experts, {MAX_TOP_K}), got {k} with {E} experts"
    if n < 1 or n * k >= 2**31:
        return f"1 <= tokens and tokens * top_k < 2^31, got {n} * {k}"
    return None


def _rows_problem(t):
    if t.dtype not in (torch.bfloat16, torch.float32):
        return f"rows must be bf16 or fp32, got {t.dtype}"
    if t.dim() != 2 or t.shape[1] == 0 or (t.shape[1] * t.element_size()) % 16:
        return f"rows must be [rows, H] with H * itemsize % 16 == 0, got {tuple(t.shape)}"
    return None


def _check(problem):
    if problem is not None:
        raise ValueError("moe: " + problem)


def moe_fused_available(x, E, k):
    """True when the HIP ops serve activations ``x`` [..., H] with E experts."""
    x2 = x.reshape(-1, x.shape[-1])
    return (use_hip(x) and _route_problem(x2.shape[0], E, k) is None
            and _rows_problem(x2) is None)


class _RouteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, k):
        logits = logits.contiguous()
        gates, idx, counts, psum, slot, row_of_slot, offsets = \
            ext().moe_route(logits, k)
        ctx.save_for_backward(logits, idx, gates)
        ctx.mark_non_differentiable(idx, counts, slot, row_of_slot, offsets)
        return gates, idx, counts, psum, slot, row_of_slot, offsets

    @staticmethod
    def backward(ctx, dgates, _didx, _dcounts, dpsum, *_):
        logits, idx, gates = ctx.saved_tensors
        # unused outputs arrive as zeros (autograd materialises them)
        return ext().moe_route_bwd(logits, idx, gates, dgates.contiguous(),
                                   dpsum.contiguous()), None


class _PermuteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot, row_of_slot, k):
        ctx.save_for_backward(slot)
        ctx.k = k
        return ext().moe_permute(x.contiguous(), row_of_slot, k)

    @staticmethod
    def backward(ctx, dxk):
        (slot,) = ctx.saved_tensors
        dx = ext().moe_combine(dxk.contiguous(), None, slot, None, ctx.k)
        return dx, None, None, None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, yk, gates, slot, row_of_slot, residual, k):
        yk = yk.contiguous()
        gates = gates.contiguous()
        ctx.save_for_backward(yk, gates, row_of_slot)
        ctx.k = k
        res = None if residual is None else residual.contiguous()
        return ext().moe_combine(yk, gates, slot, res, k)

    @staticmethod
    def backward(ctx, dy):
        yk, gates, row_of_slot = ctx.saved_tensors
        dy = dy.contiguous()
        dyk, dgates = ext().moe_combine_bwd(dy, yk, gates, row_of_slot, ctx.k)
        dres = dy if ctx.needs_input_grad[4] else None
        return dyk, dgates, None, None, dres, None


def moe_route(logits, k):
    """fp32 logits [n, E] -> (gates [n,k] f32, idx [n,k] i32, counts [E] i32,
    psum [E] f32, plan).

    The k largest logits per token in descending order (lower expert index on
    an exact tie), ``gates`` their probabilities renormalised to sum 1,
    ``counts`` the tokens per expert, ``psum`` the column sums of the full
    softmax.  Differentiable in ``gates`` and ``psum``."""
    if logits.dim() != 2:
        raise ValueError(f"moe: logits must be [n, E], got {tuple(logits.shape)}")
    n, E = logits.shape
    _check(_route_problem(n, E, k, logits.dtype))
    if use_hip(logits):
        gates, idx, counts, psum, slot, row_of_slot, offsets = \
            _RouteFn.apply(logits, k)
        return gates, idx, counts, psum, MoEPlan(slot, row_of_slot, offsets, k)
    probs = torch.softmax(logits, dim=-1)
    gates, idx = probs.topk(k, dim=-1)
    gates = gates / gates.sum(dim=-1, keepdim=True)
    flat_idx = idx.reshape(-1)
    order = torch.argsort(flat_idx, stable=True)
    slot = torch.empty_like(order)
    slot[order] = torch.arange(order.numel(), device=logits.device)
    counts = torch.bincount(flat_idx, minlength=E)
    offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    plan = MoEPlan(slot, order, offsets, k)
    return gates, idx, counts, probs.sum(dim=0), plan


def moe_permute(x, plan):
    """x [n, H] -> xk [n*k, H] with xk[s] = x[plan.row_of_slot[s] // k]."""
    _check(_rows_problem(x))
    _check(_route_problem(x.shape[0], MAX_EXPERTS, plan.k))
    if plan.slot.numel() != x.shape[0] * plan.k:
        raise ValueError("moe: plan was made for another token count")
    if use_hip(x):
        return _PermuteFn.apply(x, plan.slot, plan.row_of_slot, plan.k)
    return x.repeat_interleave(plan.k, dim=0)[plan.row_of_slot]


def moe_combine(yk, gates, plan, residual=None):
    """y[i] = sum_j gates[i,j] * yk[plan.slot[i*k+j]] (+ residual[i])."""
    _check(_rows_problem(yk))
    k = plan.k
    n = gates.shape[0]
    if yk.shape[0] != n * k or plan.slot.numel() != n * k or gates.shape[1] != k:
        raise ValueError("moe: yk, gates and plan disagree on the token count")
    if residual is not None and (residual.shape != (n, yk.shape[1])
                                 or residual.dtype != yk.dtype):
        raise ValueError("moe: residual must be [n, H] of yk's dtype")
    if use_hip(yk):
        return _CombineFn.apply(yk, gates.float(), plan.slot, plan.row_of_slot,
                                residual, k)
    y = (yk[plan.slot].reshape(n, k, -1)
         * gates.reshape(n, k, 1).to(yk.dtype)).sum(dim=1)
    if residual is not None:
        y = y + residual
    return y
