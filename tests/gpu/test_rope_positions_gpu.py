"""RoPE with per-token position ids (packed documents restart at 0)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_SEQ = 64
SHAPES = [(2, 40, 4, 64), (2, 40, 4, 128)]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _formula(x, pos, theta=10000.0):
    """fp32 rotate-half RoPE written out from the definition; pos: [b, s]."""
    hs = x.shape[-1]
    inv_freq = 1.0 / (theta ** (torch.arange(0, hs, 2, dtype=torch.float64) / hs))
    ang = pos.double().cpu()[:, :, None] * inv_freq[None, None, :]  # [b, s, hs/2]
    cos = ang.cos().float().to(x.device)[:, :, None, :]
    sin = ang.sin().float().to(x.device)[:, :, None, :]
    x1, x2 = x[..., : hs // 2], x[..., hs // 2:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_arange_positions_equal_pos0_call_bitwise(shape, dtype):
    from libai_amd.ops.rope import apply_rotary_pos_emb

    torch.manual_seed(0)
    b, s = shape[:2]
    x0 = torch.randn(*shape, device="cuda", dtype=dtype)
    g = torch.randn_like(x0)
    pos = torch.arange(s, device="cuda", dtype=torch.int32)[None].expand(b, s)
    outs = []
    for kw in (dict(pos0=0), dict(position_ids=pos)):
        x = x0.clone().requires_grad_(True)
        y = apply_rotary_pos_emb(x, MAX_SEQ, **kw)
        y.backward(g)
        outs.append((y.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_per_document_positions_match_formula(shape, dtype):
    from libai_amd.data.packing import doc_bounds_from_lengths
    from libai_amd.ops.rope import apply_rotary_pos_emb

    torch.manual_seed(1)
    b, s = shape[:2]
    # two different seeded layouts, one per batch row
    gen = torch.Generator().manual_seed(3)
    rows = []
    for _ in range(b):
        cuts = torch.randperm(s - 1, generator=gen)[:4].add(1).sort().values.tolist()
        edges = [0] + cuts + [s]
        rows.append([edges[i + 1] - edges[i] for i in range(len(edges) - 1)])
    pos = torch.stack([doc_bounds_from_lengths(r, s)[2] for r in rows]).cuda()
    assert (pos[:, 1:] < pos[:, :-1]).any(), "positions must restart somewhere"

    x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    y = apply_rotary_pos_emb(x, MAX_SEQ, position_ids=pos)
    xr = x.detach().float().requires_grad_(True)
    ref = _formula(xr, pos)
    tol = 1e-5 if dtype == torch.float32 else 1e-2  # the existing rope test's
    err = _rel(y, ref)
    print(f"{shape} {dtype} rope(position_ids) rel err {err:.3e}")
    assert err < tol
    g = torch.randn_like(y)
    y.backward(g)
    ref.backward(g.float())
    gerr = _rel(x.grad, xr.grad)
    print(f"{shape} {dtype} rope(position_ids) grad rel err {gerr:.3e}")
    assert gerr < tol * 3


@pytest.mark.parametrize("hs", [64, 128])
def test_position_ids_strided_view_input(hs):
    from libai_amd.ops.rope import apply_rotary_pos_emb

    torch.manual_seed(0)
    qkv = torch.randn(2, 40, 4, 3, hs, device="cuda", dtype=torch.bfloat16)
    pos = (torch.arange(40, device="cuda", dtype=torch.int32) % 13)[None].expand(2, 40)
    q_view = qkv[..., 0, :]
    y1 = apply_rotary_pos_emb(q_view, MAX_SEQ, position_ids=pos)
    y2 = apply_rotary_pos_emb(q_view.contiguous(), MAX_SEQ, position_ids=pos)
    assert torch.equal(y1, y2)
    assert _rel(y1, _formula(q_view.float(), pos)) < 1e-2


def test_position_ids_are_clamped_to_the_table_and_checked():
    from libai_amd.ops._ext import ext
    from libai_amd.ops.rope import _tables, apply_rotary_pos_emb

    torch.manual_seed(0)
    x = torch.randn(1, 8, 2, 64, device="cuda", dtype=torch.bfloat16)
    big = torch.full((1, 8), 10 ** 6, device="cuda", dtype=torch.int32)
    last = torch.full((1, 8), MAX_SEQ - 1, device="cuda", dtype=torch.int32)
    assert torch.equal(apply_rotary_pos_emb(x, MAX_SEQ, position_ids=big),
                       apply_rotary_pos_emb(x, MAX_SEQ, position_ids=last))
    with pytest.raises(ValueError):
        apply_rotary_pos_emb(x, MAX_SEQ, pos0=3, position_ids=last)
    cos_t, sin_t = _tables(MAX_SEQ, 64, 10000.0, x.device)
    with pytest.raises(RuntimeError, match="pos_ids"):
        ext().rope(x, cos_t, sin_t, 0, False, last.long())
    with pytest.raises(RuntimeError, match="pos_ids"):
        ext().rope(x, cos_t, sin_t, 0, False, last[:, :4].contiguous())
