"""The HIP MoE ops (csrc/kernels/moe.hip) against fp64 evaluations of the
layer's formulas, and MoELayer(fused_dispatch=True) against the unfused layer."""

import copy

import pytest
import torch

from libai_amd.ops.moe import moe_combine, moe_permute, moe_route

pytestmark = pytest.mark.gpu

# (n, E, k): several tokens per wave + ragged last wave + 4 workgroups; the
# narrowest group; one token per wave (3 workgroups); >1 expert per lane
ROUTE_CASES = [(200, 8, 2), (77, 4, 1), (130, 64, 4), (65, 160, 2)]
# routings for the plan / permute / combine tests: random, every copy on one
# expert, an expert that receives nothing (k = 5 takes the 8-row combine)
PLAN_CASES = ["random", "one_expert", "empty_expert"]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _logits(n, E, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, E, generator=g)


def _ref_route(logits, k, wg, dtype):
    """The layer's formulation in `dtype`: gates, idx, psum and the gradient of
    sum(gates * wg) + E * sum(frac * psum / n) w.r.t. the logits."""
    lg = logits.to(dtype).clone().requires_grad_()
    n, E = lg.shape
    probs = torch.softmax(lg, dim=-1)
    gates, idx = probs.topk(k, dim=-1)
    gates = gates / gates.sum(dim=-1, keepdim=True)
    psum = probs.sum(0)
    frac = torch.bincount(idx.reshape(-1), minlength=E).to(dtype) / (n * k)
    ((gates * wg.to(dtype)).sum() + E * (frac * psum / n).sum()).backward()
    return gates.detach(), idx, psum.detach(), lg.grad


@pytest.mark.parametrize("n,E,k", ROUTE_CASES)
def test_route_fwd_bwd(n, E, k):
    logits = _logits(n, E).cuda()
    wg = _logits(n, k, seed=1).cuda()
    top = logits.double().topk(min(k + 1, E)).values
    assert (top[:, :-1] > top[:, 1:]).all()  # no ties among the top k + 1
    g64, idx64, p64, d64 = _ref_route(logits, k, wg, torch.float64)
    g32, _, p32, d32 = _ref_route(logits, k, wg, torch.float32)

    lg = logits.clone().requires_grad_()
    gates, idx, counts, psum, plan = moe_route(lg, k)
    frac = counts.float() / (n * k)
    ((gates * wg).sum() + E * (frac * psum / n).sum()).backward()

    assert torch.equal(idx.long(), idx64)
    assert torch.equal(counts.long(), torch.bincount(idx64.reshape(-1), minlength=E))
    for name, got, t32, ref in (("gates", gates, g32, g64), ("psum", psum, p32, p64),
                                ("dlogits", lg.grad, d32, d64)):
        err = (got.double() - ref).abs().max().item()
        err_torch = (t32.double() - ref).abs().max().item()
        print(f"route {(n, E, k)} {name}: err {err:.3e} torch fp32 {err_torch:.3e}")
        assert err <= 2 * err_torch, (name, err, err_torch)


def test_route_all_zero_logits():
    gates, idx, counts, _, _ = moe_route(torch.zeros(70, 8, device="cuda"), 3)
    assert torch.equal(idx, torch.arange(3, device="cuda", dtype=torch.int32)
                       .expand(70, 3))
    assert torch.equal(gates, torch.full((70, 3), 1 / 3, device="cuda"))
    assert counts.tolist() == [70, 70, 70, 0, 0, 0, 0, 0]


def _routing(kind):
    if kind == "random":
        return moe_route(_logits(200, 8).cuda(), 2)
    if kind == "one_expert":
        lg = _logits(150, 8)
        lg[:, 3] = 10.0
        return moe_route(lg.cuda(), 1)
    lg = _logits(130, 6)
    lg[:, 2] = -30.0
    return moe_route(lg.cuda(), 5)


@pytest.mark.parametrize("kind", PLAN_CASES)
def test_plan_is_stable_sort(kind):
    _, idx, counts, _, plan = _routing(kind)
    order = torch.argsort(idx.reshape(-1).long(), stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel(), device="cuda")
    assert torch.equal(plan.slot.long(), inv)
    assert torch.equal(plan.row_of_slot.long(), order)
    assert plan.expert_offsets.tolist() == [0] + counts.cumsum(0).tolist()
    if kind == "one_expert":
        assert counts.tolist() == [0, 0, 0, 150, 0, 0, 0, 0]
    if kind == "empty_expert":
        assert counts[2].item() == 0


@pytest.mark.parametrize("H", [72, 1032])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", PLAN_CASES)
def test_permute_fwd_bwd(kind, dtype, H):
    _, idx, _, _, plan = _routing(kind)
    n, k = idx.shape
    torch.manual_seed(2)
    x = torch.randn(n, H, device="cuda").to(dtype).requires_grad_()
    xk = moe_permute(x, plan)
    assert torch.equal(xk, x.detach().repeat_interleave(k, 0)[plan.row_of_slot.long()])

    dxk = torch.randn(n * k, H, device="cuda").to(dtype)
    xk.backward(dxk)
    terms = dxk.double()[plan.slot.long()].reshape(n, k, H)
    # k - 1 fp32 additions, then one rounding to the output dtype
    tol = terms.abs().sum(1) * (k * 2.0**-23 + (2.0**-8 if dtype == torch.bfloat16
                                                else 2.0**-23))
    assert ((x.grad.double() - terms.sum(1)).abs() <= tol).all()


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("H", [72, 1032])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("kind", PLAN_CASES)
def test_combine_fwd_bwd(kind, dtype, H, with_res):
    gates, idx, _, _, plan = _routing(kind)
    n, k = idx.shape
    torch.manual_seed(3)
    yk = torch.randn(n * k, H, device="cuda").to(dtype).requires_grad_()
    gates = gates.detach().requires_grad_()
    res = torch.randn(n, H, device="cuda").to(dtype).requires_grad_() \
        if with_res else None
    dy = torch.randn(n, H, device="cuda").to(dtype)
    y = moe_combine(yk, gates, plan, res)
    y.backward(dy)

    rel = 2.0**-8 if dtype == torch.bfloat16 else 2.0**-22 * k
    g64 = gates.detach().double()
    rows = yk.detach().double()[plan.slot.long()].reshape(n, k, H)
    terms = g64[:, :, None] * rows
    ref = terms.sum(1) + (res.detach().double() if with_res else 0)
    mag = terms.abs().sum(1) + (res.detach().double().abs() if with_res else 0)
    # one output rounding + the fp32 accumulation of k (+1) terms
    assert ((y.double() - ref).abs() <= rel * ref.abs() + (k + 1) * 2.0**-23 * mag).all()

    dy_rows = dy.double()[:, None, :].expand(n, k, H)
    ref_dyk = (g64[:, :, None] * dy_rows).reshape(n * k, H)[plan.row_of_slot.long()]
    assert ((yk.grad.double() - ref_dyk).abs() <= rel * ref_dyk.abs()).all()
    prod = dy_rows * rows
    assert ((gates.grad.double() - prod.sum(-1)).abs()
            <= H * 2.0**-23 * prod.abs().sum(-1)).all()
    if with_res:
        assert torch.equal(res.grad, dy)


def _layer_run(layer, x):
    x = x.clone().requires_grad_()
    y = layer(x)
    (y.float().pow(2).mean() + layer.last_aux_loss).backward()
    grads = [p.grad for p in (layer.router.weight, layer.w1, layer.w2)] + [x.grad]
    return [y.detach()] + grads, layer.last_aux_loss.detach()


def test_layer_fused_matches_unfused():
    from libai_amd.layers.moe import MoELayer

    torch.manual_seed(0)
    fused = MoELayer(64, 128, num_experts=4, top_k=2, fused_dispatch=True).cuda()
    plain = copy.deepcopy(fused)
    plain.fused_dispatch = False
    plain64 = copy.deepcopy(plain).double()
    x = torch.randn(2, 48, 64, device="cuda")
    logits = torch.nn.functional.linear(x.reshape(-1, 64), plain.router.weight)
    assert torch.equal(moe_route(logits.detach(), 2)[1].long(),
                       logits.softmax(-1).topk(2).indices)  # the chosen experts

    out_f, aux_f = _layer_run(fused, x)
    out_p, aux_p = _layer_run(plain, x)
    out_64, aux_64 = _layer_run(plain64, x.double())
    # the aux loss is a sum of 4 products of fp32 sums over 96 tokens
    assert abs(aux_f.item() - aux_p.item()) <= 96 * 2.0**-23 * abs(aux_64.item())
    for name, f, p, r in zip(("y", "d_router", "d_w1", "d_w2", "dx"),
                             out_f, out_p, out_64):
        diff = (f - p).abs().max().item()
        own = (p.double() - r).abs().max().item()
        print(f"layer {name}: fused - unfused {diff:.3e}, unfused - fp64 {own:.3e}")
        assert diff <= 2 * own, (name, diff, own)

    y_f = fused.bfloat16()(x.bfloat16()).float()
    y_p = plain.bfloat16()(x.bfloat16()).float()
    assert torch.isfinite(y_f).all()
    assert (y_f - y_p).abs().max() <= 2.0**-7 * y_p.abs().max()
