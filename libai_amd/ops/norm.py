"""LayerNorm / RMSNorm functional ops: HIP kernels on GPU, torch reference on CPU.

Replaces the reference's flow._C.layer_norm_affine / flow._C.rms_norm
(reference: libai/layers/layer_norm.py:78-131).

``layer_norm_residual`` / ``bias_dropout_add_norm`` are the training forms for
a pre-LN residual stream: the norm hands its input on as a second output (the
residual), so that the gradient arriving on the residual branch reaches the
norm's backward kernel and is added there instead of by a separate add.
"""

import torch
import torch.nn.functional as F

from ._ext import draw_seed, ext, use_hip
from .fused_bias import bias_dropout_add

__all__ = ["layer_norm", "rms_norm", "layer_norm_residual",
           "bias_dropout_add_norm", "res_norm_fusable"]


class _NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, rms):
        x = x.contiguous()
        y, mean, rstd = ext().ln_fwd(x, weight.contiguous(),
                                     bias.contiguous() if bias is not None else None,
                                     rms, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.rms = rms
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = ext().ln_bwd(
            dy.contiguous(), x, weight, mean, rstd, ctx.rms, ctx.has_bias
        )
        return dx, dgamma, (dbeta if ctx.has_bias else None), None, None


def layer_norm(x, weight, bias, eps=1e-5):
    if use_hip(x):
        return _NormFn.apply(x, weight, bias, eps, False)
    return F.layer_norm(x, (weight.numel(),), weight, bias, eps)


def _rms_norm_ref(x, weight, eps):
    dt = x.dtype
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * rstd).to(dt) * weight


def rms_norm(x, weight, eps=1e-5):
    if use_hip(x):
        return _NormFn.apply(x, weight, None, eps, True)
    return _rms_norm_ref(x, weight, eps)


class _NormResFn(torch.autograd.Function):
    """(y, x) = norm(x): x comes back as an output (autograd aliases it, no
    copy), so its gradient -- the residual branch -- arrives in backward next
    to dy and the kernel writes bf16(bf16(dx_ln) + dres) in one pass."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, rms):
        assert x.is_contiguous()
        y, mean, rstd = ext().ln_fwd(x, weight.contiguous(),
                                     bias.contiguous() if bias is not None else None,
                                     rms, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.rms = rms
        ctx.has_bias = bias is not None
        ctx.set_materialize_grads(False)
        return y, x

    @staticmethod
    def backward(ctx, dy, dres):
        if dy is None:  # only the pass-through was used
            return dres, None, None, None, None
        x, weight, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = ext().ln_bwd(
            dy.contiguous(), x, weight, mean, rstd, ctx.rms, ctx.has_bias,
            dres.contiguous() if dres is not None else None,
        )
        return dx, dgamma, (dbeta if ctx.has_bias else None), None, None


def layer_norm_residual(x, weight, bias, eps=1e-5, rms=False):
    """Returns (norm(x), x).  Use the second output as the residual."""
    if use_hip(x) and x.is_contiguous():
        return _NormResFn.apply(x, weight, bias, eps, rms)
    y = rms_norm(x, weight, eps) if rms else layer_norm(x, weight, bias, eps)
    return y, x


def res_norm_fusable(x, weight):
    """Whether bias_dropout_add_norm runs as one kernel for this input: bf16
    on the GPU and a width on the norm kernels' wave path (whole 16-byte
    vectors, at most 4 per lane)."""
    H = x.shape[-1]
    return (
        use_hip(x)
        and x.dtype == torch.bfloat16
        and weight is not None
        and weight.dtype == torch.bfloat16
        and H % 8 == 0
        and 8 <= H <= 2048
        and x.numel() > 0
    )


class _BiasDropoutAddNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, weight, beta, eps, rms, p):
        x = x.contiguous()
        b = bias.contiguous() if bias is not None else None
        bt = beta.contiguous() if beta is not None else None
        # drawn here, once, where bias_dropout_add draws it: a seeded run
        # consumes the same seed sequence with and without the fusion
        seed = draw_seed() if p > 0 else 0
        h, y, mean, rstd = ext().res_drop_norm_fwd(
            x, b, residual.contiguous(), weight.contiguous(), bt, eps, rms, p, seed
        )
        ctx.save_for_backward(h, weight, mean, rstd)
        ctx.p = p
        ctx.seed = seed
        ctx.rms = rms
        ctx.has_bias = b is not None
        ctx.has_beta = bt is not None
        ctx.set_materialize_grads(False)
        return h, y

    @staticmethod
    def backward(ctx, dres, dy):
        h, weight, mean, rstd = ctx.saved_tensors
        if dy is None:  # y unused: nothing flows through the norm
            if dres is None:
                return (None,) * 8
            dy = torch.zeros_like(h)
        dh, dx, dgamma, dbeta, dbias = ext().res_drop_norm_bwd(
            dy.contiguous(), h, weight.contiguous(), mean, rstd,
            dres.contiguous() if dres is not None else None,
            ctx.rms, ctx.has_beta, ctx.has_bias, ctx.p, ctx.seed,
        )
        return dx, dbias, dh, dgamma, dbeta, None, None, None


def bias_dropout_add_norm(x, bias, residual, weight, norm_bias, eps=1e-5, p=0.0,
                          training=True, rms=False):
    """h = residual + dropout(x + bias); y = norm(h).  Returns (h, y).

    One kernel forward and one backward where ``res_norm_fusable``; otherwise
    (CPU, fp32, wide or ragged rows) the composition of the separate ops,
    which is also what the fused kernels are tested against bit for bit."""
    if res_norm_fusable(x, weight):
        return _BiasDropoutAddNormFn.apply(
            x, bias, residual, weight, None if rms else norm_bias, eps, rms,
            p if training else 0.0,
        )
    h = bias_dropout_add(x, bias=bias, residual=residual, p=p, training=training)
    if rms:
        return h, rms_norm(h, weight, eps)
    return h, layer_norm(h, weight, norm_bias, eps)
