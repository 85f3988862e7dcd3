"""Fused bias+gelu and bias+dropout+residual ops.

Replaces the reference's flow._C.fused_bias_add_gelu (libai/layers/mlp.py:95-97)
and flow._C.fused_bias_add_dropout (+ the residual add that follows it in
TransformerLayer; reference: libai/layers/attention.py:265-267,
libai/layers/transformer_layer.py:170-232).
"""

import torch
import torch.nn.functional as F

from ._ext import draw_seed, ext, use_hip

__all__ = ["bias_gelu", "bias_dropout_add"]


def _kernel_width(x, op):
    """The kernels index rows in whole 16-byte vectors (8 bf16 / 4 fp32), so
    they serve widths that are a multiple of 8.  Any other width runs the
    composed torch path; this is a SHAPE fallback, not an extension fallback
    -- log it once so it cannot hide silently."""
    if x.shape[-1] > 0 and x.shape[-1] % 8 == 0:
        return True
    import logging

    from ..utils.logger import log_first_n

    log_first_n(
        logging.WARNING,
        f"{op}: width {x.shape[-1]} is not a multiple of 8; using the "
        f"composed torch path for this shape",
        n=1,
        key=f"{op}_ragged_width",
    )
    return False


class _BiasGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        x = x.contiguous()
        b = bias.contiguous() if bias is not None else None
        y = ext().bias_gelu_fwd(x, b)
        ctx.save_for_backward(x, *( (b,) if b is not None else () ))
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.has_bias:
            x, b = ctx.saved_tensors
        else:
            (x,) = ctx.saved_tensors
            b = None
        dy = dy.contiguous()
        # the bias grad partials ride in the same kernel pass (no re-read
        # of dx); ragged widths never get here (see _kernel_width)
        dx, dbias = ext().bias_gelu_bwd(x, b, dy, ctx.has_bias)
        if ctx.has_bias and dbias is None:
            dbias = ext().colsum(dx, x.shape[-1])
        return dx, dbias


def bias_gelu(x, bias=None):
    """y = gelu(x + bias) with exact-erf gelu (torch default)."""
    if use_hip(x) and _kernel_width(x, "bias_gelu"):
        return _BiasGeluFn.apply(x, bias)
    return F.gelu(x + bias if bias is not None else x)


class _BiasDropoutAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, p):
        x = x.contiguous()
        b = bias.contiguous() if bias is not None else None
        r = residual.contiguous() if residual is not None else None
        seed = draw_seed() if p > 0 else 0
        y = ext().bias_dropout_res_fwd(x, b, r, p, seed)
        ctx.p = p
        ctx.seed = seed
        ctx.has_bias = b is not None
        ctx.has_res = r is not None
        ctx.width = x.shape[-1]
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dbias = None
        if ctx.p > 0:
            dx, dbias = ext().bias_dropout_res_bwd(dy, ctx.p, ctx.seed,
                                                   ctx.has_bias)
        else:
            dx = dy
        if ctx.has_bias and dbias is None:
            dbias = ext().colsum(dx, ctx.width)
        dres = dy if ctx.has_res else None
        return dx, dbias, dres, None


def bias_dropout_add(x, bias=None, residual=None, p=0.0, training=True):
    """y = residual + dropout(x + bias).  Philox-recomputed mask (no mask tensor)."""
    if use_hip(x) and _kernel_width(x, "bias_dropout_add"):
        return _BiasDropoutAddFn.apply(x, bias, residual, p if training else 0.0)
    out = x + bias if bias is not None else x
    out = F.dropout(out, p=p, training=training)
    if residual is not None:
        out = out + residual
    return out
