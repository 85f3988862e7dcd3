"""Fused residual chain (kernels/res_norm.hip) against the separate kernels.

Activations and activation gradients (h, y, dx, the residual gradient) must be
bit-identical to the chain bias_dropout_add -> layer_norm / rms_norm with
autograd's add.  dgamma / dbeta / dbias change in summation order only: each
form is compared with an fp64 composition of the same bf16 inputs on the CPU,
and the fused form's maximum error may exceed the unfused form's by at most
one bf16 ulp of that gradient's largest magnitude (a different order of fp32
partials can flip the final rounding to bf16 and nothing more).

Shapes: H 64 (fewer vectors than lanes), 1024 (2 per lane), 1032 (4 per lane,
idle lanes), 2048 (4 full), 1004 (ragged: existing path); R 1, 5 (not a
multiple of the waves per block) and row counts above the number of waves the
backward starts (at most 1024 blocks x 4 waves) that are no multiple of it.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = [(1, 64), (5, 64), (9001, 64), (1, 1024), (5, 1024), (9001, 1024),
          (5, 1032), (300, 1032), (5, 2048), (4501, 2048), (5, 1004), (300, 1004)]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    from libai_amd.ops._ext import has_ext

    assert has_ext(), "HIP extension must be built+loaded on the GPU box"
    yield


def _bf16_ulp(mag):
    """Spacing of bf16 (8 significand bits) at magnitude ``mag``."""
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - 7)


def _check_param_grad(name, fused, unfused, ref64):
    """Both against the fp64 reference; fused may be worse by one bf16 ulp of
    the gradient's largest magnitude.  Prints the pair of errors."""
    ef = (fused.double().cpu() - ref64).abs().max().item()
    eu = (unfused.double().cpu() - ref64).abs().max().item()
    ulp = _bf16_ulp(ref64.abs().max().item())
    print(f"    {name}: err fused {ef:.3e} unfused {eu:.3e} (ulp {ulp:.3e})")
    assert ef <= eu + ulp, (name, ef, eu, ulp)


def _inputs(R, H, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device="cuda", generator=g) * scale).to(torch.bfloat16)

    return dict(x=rn(R, H), bias=rn(H, scale=0.5), res=rn(R, H, scale=2.0),
                w=rn(H) + 1, b=rn(H, scale=0.3), gy=rn(R, H), gh=rn(R, H))


def _chain(fused, d, rms, p, with_bias, with_dres):
    """One forward + backward of the chain; returns tensors by name."""
    from libai_amd.ops.fused_bias import bias_dropout_add
    from libai_amd.ops.norm import bias_dropout_add_norm, layer_norm, rms_norm

    torch.manual_seed(1234)  # draw_seed() returns the same seed in both arms
    x = d["x"].clone().requires_grad_(True)
    res = d["res"].clone().requires_grad_(True)
    bias = d["bias"].clone().requires_grad_(True) if with_bias else None
    w = d["w"].clone().requires_grad_(True)
    b = None if rms else d["b"].clone().requires_grad_(True)
    if fused:
        h, y = bias_dropout_add_norm(x, bias, res, w, b, EPS, p=p, training=True,
                                     rms=rms)
    else:
        h = bias_dropout_add(x, bias=bias, residual=res, p=p, training=True)
        y = rms_norm(h, w, EPS) if rms else layer_norm(h, w, b, EPS)
    if with_dres:
        torch.autograd.backward([y, h], [d["gy"], d["gh"]])
    else:
        torch.autograd.backward([y], [d["gy"]])
    out = dict(h=h.detach(), y=y.detach(), dx=x.grad, dres=res.grad, dgamma=w.grad)
    if bias is not None:
        out["dbias"] = bias.grad
    if b is not None:
        out["dbeta"] = b.grad
    return out


def _ref64(d, h, dx, rms, with_bias):
    """fp64 composition on the CPU from the bf16 tensors the kernels read
    (h, dy) and wrote (dx: its column sum is dbias)."""
    h64 = h.double().cpu()
    dy = d["gy"].double().cpu()
    if rms:
        xhat = h64 * torch.rsqrt(h64.pow(2).mean(-1, keepdim=True) + EPS)
    else:
        mu = h64.mean(-1, keepdim=True)
        xhat = (h64 - mu) * torch.rsqrt(h64.var(-1, unbiased=False, keepdim=True) + EPS)
    ref = dict(dgamma=(dy * xhat).sum(0))
    if not rms:
        ref["dbeta"] = dy.sum(0)
    if with_bias:
        # dbias sums dres * keep before its rounding to dx; keep is 0 or the
        # fp32 scale, so recover the mask from dx and redo the product in fp64
        ref["dbias_mask"] = dx.double().cpu() != 0
    return ref


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("R,H", SHAPES)
def test_fused_chain_matches_separate_kernels(R, H, rms, p):
    d = _inputs(R, H)
    for with_bias in (True, False):
        for with_dres in (True, False):
            print(f"  R={R} H={H} rms={rms} p={p} bias={with_bias} dres={with_dres}")
            f = _chain(True, d, rms, p, with_bias, with_dres)
            u = _chain(False, d, rms, p, with_bias, with_dres)
            for k in ("h", "y", "dx", "dres"):
                assert torch.equal(f[k], u[k]), (k, with_bias, with_dres)
            ref = _ref64(d, u["h"], u["dx"], rms, with_bias)
            _check_param_grad("dgamma", f["dgamma"], u["dgamma"], ref["dgamma"])
            if not rms:
                _check_param_grad("dbeta", f["dbeta"], u["dbeta"], ref["dbeta"])
            if with_bias:
                scale = float(torch.tensor(1.0, dtype=torch.float32) /
                              (torch.tensor(1.0, dtype=torch.float32) -
                               torch.tensor(p, dtype=torch.float32)))
                dh64 = u["dres"].double().cpu()
                if p > 0:
                    db = (dh64 * ref["dbias_mask"] * scale).sum(0)
                else:
                    db = dh64.sum(0)
                _check_param_grad("dbias", f["dbias"], u["dbias"], db)


def _ln_bwd_both(dtype, R, H, rms, with_dres):
    from libai_amd.ops._ext import ext

    g = torch.Generator(device="cuda").manual_seed(3)
    x = (torch.randn(R, H, device="cuda", generator=g) * 2 + 0.5).to(dtype)
    dy = torch.randn(R, H, device="cuda", generator=g).to(dtype)
    w = (torch.randn(H, device="cuda", generator=g) + 1).to(dtype)
    b = None if rms else torch.zeros(H, device="cuda", dtype=dtype)
    dres = torch.randn(R, H, device="cuda", generator=g).to(dtype) if with_dres else None
    _, mean, rstd = ext().ln_fwd(x, w, b, rms, EPS)
    new = ext().ln_bwd(dy, x, w, mean, rstd, rms, not rms, dres, True)
    old = ext().ln_bwd(dy, x, w, mean, rstd, rms, not rms, None, False)
    old_dx = old[0] + dres if with_dres else old[0]  # the add autograd launched
    return x, dy, new, (old_dx, old[1], old[2])


@pytest.mark.parametrize("with_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("R,H", SHAPES)
def test_single_pass_ln_bwd_matches_kernel_pair(R, H, rms, with_dres):
    """dx of the single-pass kernel against the dx + wgrad_partial pair that
    it replaces (still built: ``single_pass=False``; H=1004 runs the pair in
    both arms, with the residual gradient added by torch)."""
    x, dy, new, old = _ln_bwd_both(torch.bfloat16, R, H, rms, with_dres)
    assert torch.equal(new[0], old[0])
    x64, dy64 = x.double().cpu(), dy.double().cpu()
    if rms:
        xhat = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + EPS)
    else:
        xhat = (x64 - x64.mean(-1, keepdim=True)) * torch.rsqrt(
            x64.var(-1, unbiased=False, keepdim=True) + EPS)
    print(f"  R={R} H={H} rms={rms} dres={with_dres}")
    _check_param_grad("dgamma", new[1], old[1], (dy64 * xhat).sum(0))
    if not rms:
        _check_param_grad("dbeta", new[2], old[2], dy64.sum(0))


@pytest.mark.parametrize("R,H", [(5, 64), (300, 1024), (9001, 512)])
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_single_pass_ln_bwd_fp32(R, H, rms):
    """fp32 rows take the single-pass kernel too (4 floats per vector, wave
    path up to H = 1024).  dx: same expressions, so equal.  dgamma / dbeta:
    two fp32 summation orders of R terms each stay within R * 2^-24 *
    sum|terms| of the exact sum, so within twice that of each other."""
    x, dy, new, old = _ln_bwd_both(torch.float32, R, H, rms, True)
    assert torch.equal(new[0], old[0])
    x64, dy64 = x.double().cpu(), dy.double().cpu()
    if rms:
        xhat = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + EPS)
    else:
        xhat = (x64 - x64.mean(-1, keepdim=True)) * torch.rsqrt(
            x64.var(-1, unbiased=False, keepdim=True) + EPS)
    bound = 2 * R * 2.0 ** -24 * (dy64 * xhat).abs().sum(0)
    assert ((new[1].double().cpu() - old[1].double().cpu()).abs() <= bound).all()
    if not rms:
        bound = 2 * R * 2.0 ** -24 * dy64.abs().sum(0)
        assert ((new[2].double().cpu() - old[2].double().cpu()).abs() <= bound).all()


def test_pass_through_is_an_alias_not_a_copy():
    from libai_amd.ops.norm import layer_norm_residual

    x = torch.randn(7, 1024, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    w = torch.ones(1024, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    b = torch.zeros(1024, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    y, x2 = layer_norm_residual(x, w, b, EPS)
    assert x2.data_ptr() == x.data_ptr() and x2.grad_fn is not None
    # only the pass-through used / only the norm used
    (gx,) = torch.autograd.grad(x2.sum(), x, retain_graph=True)
    assert torch.equal(gx, torch.ones_like(x))
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad.float()).all()


def _layer(hidden, heads, p):
    from libai_amd.layers.attention import AttnMaskType
    from libai_amd.layers.transformer_layer import TransformerLayer

    torch.manual_seed(0)
    return TransformerLayer(
        hidden, 4 * hidden, heads, attention_dropout_prob=p, output_dropout_prob=p,
        attn_mask_type=AttnMaskType.causal,
    ).to(torch.bfloat16).cuda().train()


def _layer_run(layer, x0, g, fused, ckpt):
    from torch.utils.checkpoint import checkpoint

    layer.fuse_residual_norm = fused
    layer.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(77)
    y = checkpoint(layer, x, use_reentrant=False) if ckpt else layer(x)
    y.backward(g)
    return y.detach(), x.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


@pytest.mark.parametrize("ckpt", [False, True], ids=["plain", "checkpointed"])
def test_layer_switch_on_matches_off(ckpt):
    layer = _layer(256, 4, 0.1)
    g = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.randn(3, 128, 256, device="cuda", generator=g).to(torch.bfloat16)
    gy = torch.randn(3, 128, 256, device="cuda", generator=g).to(torch.bfloat16)
    y1, dx1, pg1 = _layer_run(layer, x0, gy, True, ckpt)
    y0, dx0, pg0 = _layer_run(layer, x0, gy, False, ckpt)
    assert torch.equal(y1, y0)
    assert torch.equal(dx1, dx0)
    # both arms round nearly the same fp32 sum to bf16: at most one ulp of
    # the gradient's largest magnitude apart (GEMM weight grads: identical
    # inputs, so equal)
    for n in pg0:
        diff = (pg1[n].float() - pg0[n].float()).abs().max().item()
        ulp = _bf16_ulp(pg0[n].float().abs().max().item())
        assert diff <= ulp, (n, diff, ulp)


# Parent-vs-parent difference of the last loss of `bench.py --dump-outputs
# --steps 5 --warmup 2`: six runs of the parent build on one box on the day of
# this change, the largest of their 15 pairwise differences
# (profiles/res_norm_fused.md, "Results unchanged").  It is what run-to-run
# noise (float atomics, per-process library choices) already does to that
# loss.  One pair is not enough to know it: the 15 pairs range from 0 to
# 3.6e-5, and a first single pair happened to give 3.8e-6.
LOSS_NOISE = 3.624e-5


def test_gpt_three_steps_switch_on_matches_off():
    """Three optimizer steps of a 2-layer GPT with the bench's settings
    (hidden 1024, 16 heads, sequence 1024, vocabulary 50304, dropout 0.1,
    bf16, AdamW 1.5e-4 / 0.01 with clipping at 1.0) at micro-batch 4.

    The first loss must be equal: every activation is bit-identical.  The
    later ones may differ by the noise above, because dgamma, dbeta and the
    attention dbias differ in their last bf16 bit (fp32 partials summed in
    another order; the layer test above bounds that by one ulp) and the
    optimizer carries those bits on.  Measured on MI355X boxes, both forms in
    one process: 2.9e-5 / 2.4e-5, 0 / 7.6e-6, 2.9e-5 / 2.2e-5 at steps 2 / 3.
    For scale: the parent build, run four times on this very workload in
    processes of its own, gave 11.0346613 or 11.0346947 at step 2 (3.3e-5
    apart) and 11.0227680 to 11.0228586 at step 3 (9.1e-5)."""
    from libai_amd.models import GPTForPreTraining
    from libai_amd.optim import FusedAdamW, get_default_optimizer_params

    def run(fused):
        torch.manual_seed(1234)
        model = GPTForPreTraining(
            hidden_layers=2, vocab_size=50304, hidden_size=1024,
            ffn_hidden_size=4096, num_attention_heads=16, max_seq_length=1024,
            attention_dropout_prob=0.1, output_dropout_prob=0.1,
        ).to(torch.bfloat16).cuda().train()
        for m in model.modules():
            if hasattr(m, "fuse_residual_norm"):
                m.fuse_residual_norm = fused
        opt = FusedAdamW(
            get_default_optimizer_params(model, base_lr=1.5e-4, weight_decay=0.01),
            lr=1.5e-4, weight_decay=0.01, clip_grad=1.0)
        g = torch.Generator(device="cuda").manual_seed(4321)
        losses = []
        for _ in range(3):
            ids = torch.randint(0, 50304, (4, 1025), device="cuda", generator=g)
            loss = sum(model(input_ids=ids[:, :-1], labels=ids[:, 1:]).values())
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.detach().float().cpu())
        return losses

    on, off = run(True), run(False)
    print("  losses on ", [f"{float(v):.7f}" for v in on])
    print("  losses off", [f"{float(v):.7f}" for v in off])
    assert torch.equal(on[0], off[0])  # one forward: nothing may differ
    for a, b in zip(on[1:], off[1:]):
        assert torch.equal(a, b) or abs(float(a) - float(b)) <= LOSS_NOISE
