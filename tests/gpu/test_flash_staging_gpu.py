"""K/V staging of flash_fwd and flash_bwd_q: global loads split from LDS stores.

The round loop of the forward (128 keys) and the tile loop of the dQ backward
(64 keys at D = 64, 32 at D = 128) issue every global load of a round into
registers, rows clamped to Sk - 1 and zeros selected afterwards, and only then
write the LDS images.  The shapes are the ones at which such a loop can go
wrong: one round, a last round of 8 valid rows (GQA 4 on 2), three ragged
rounds, Sq != Sk, staged rows past kv_len, a loop that starts at a later round
(window 40, packed documents), the rel_bias table staged between the same
barriers, dropout, and a ragged key count behind a query offset (forward only:
the clamp row is Sk - 1 = 116, not a multiple of 8).

Every case has two oracles, neither of them the code under test:

1. an fp32 PyTorch reference, within the project's bounds: 2e-2 max-abs
   forward and 5e-2 of the reference gradient's max-abs
   (tests/gpu/test_flash_attn_gpu.py); with dropout the reference applies the
   oracle's mask (tests/dropout_oracle.py) and the forward bound is divided by
   1 - p (tests/gpu/test_dropout_exact_gpu.py);
2. the bits of O, lse, dQ, dK and dV recorded from the build before the
   staging was split (tools/make_flash_golden.py ->
   tests/golden/flash_stage_*.npz), required to be equal.  The rel_bias
   table's gradient is summed with atomics and is checked against the
   reference only.

Each case runs the kernels once; both tests read the shared result.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.dropout_oracle import attn_keep_mask, keep_scale

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2
GRAD_TOL = 5e-2

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _golden_tool():
    spec = importlib.util.spec_from_file_location(
        "make_flash_golden", os.path.join(ROOT, "tools", "make_flash_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TOOL = _golden_tool()
CASES = list(_TOOL.cases())


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    from libai_amd.ops._ext import has_ext

    assert has_ext(), "HIP extension must be built+loaded on the GPU box"
    yield


_RESULTS = {}


def _run(c):
    """(inputs on the device, kernel outputs) of case c; computed once"""
    if c["name"] not in _RESULTS:
        from libai_amd.ops._ext import ext

        t = {k: (v.cuda() if v is not None else None)
             for k, v in _TOOL.make_inputs(c).items()}
        _RESULTS[c["name"]] = (t, _TOOL.run_case(ext(), c, t))
    return _RESULTS[c["name"]]


def _reference(c, t):
    """fp32 O [B, Sq, H, D] with autograd leaves (q, k, v, table or None).
    Query i sits at position q_offset + i and sees key j iff j < kv_len[b],
    j <= position when causal, position - j < window, j >= doc_start[b][i];
    rel_bias adds table[h, j - i + Sq - 1]; dropout multiplies the
    probabilities by the oracle's keep mask over 1 - p."""
    b, h, hkv, sq, sk = (c[x] for x in ("b", "h", "hkv", "sq", "sk"))
    scale = _TOOL.scale_of(c)
    q, k, v = (t[n].detach().float().requires_grad_(True) for n in ("q", "k", "v"))
    table = t["table"].detach().clone().requires_grad_(True) if c["rel_bias"] else None
    qh = q.permute(0, 2, 1, 3)
    kh = k.repeat_interleave(h // hkv, dim=2).permute(0, 2, 1, 3)
    vh = v.repeat_interleave(h // hkv, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    i = torch.arange(sq, device="cuda")[:, None]
    j = torch.arange(sk, device="cuda")[None, :]
    pos = i + c["q_offset"]
    if table is not None:
        s = s + table[:, j - i + (sq - 1)][None]
    vis = torch.ones(sq, sk, dtype=torch.bool, device="cuda")
    if c["causal"]:
        vis = vis & (j <= pos)
    if c["window"]:
        vis = vis & (pos - j < c["window"])
    vis = vis[None, None].expand(b, 1, sq, sk)
    if t["kv_len"] is not None:
        vis = vis & (j[None, None] < t["kv_len"].long()[:, None, None, None])
    if t["doc_start"] is not None:
        vis = vis & (j[None, None] >= t["doc_start"].long()[:, None, :, None])
    s = s.masked_fill(~vis, float("-inf"))
    has_key = vis.any(-1, keepdim=True)
    s = torch.where(has_key, s, torch.zeros_like(s))  # keep empty rows finite
    p = torch.softmax(s, dim=-1) * has_key
    if c["p"] > 0:
        keep = attn_keep_mask(_TOOL.DROP_SEED, b * h, sq, sk, c["p"]).view(b, h, sq, sk)
        p = p * keep.cuda().float() * float(keep_scale(c["p"]))
    return torch.matmul(p, vh).permute(0, 2, 1, 3), (q, k, v, table)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_matches_fp32_reference(c):
    t, res = _run(c)
    ref, (q, k, v, table) = _reference(c, t)
    tag = f"[flash-staging] {c['name']}"
    failures = []
    assert torch.isfinite(res["o"].float()).all(), f"{tag}: forward not finite"
    bound = FWD_TOL / (1 - c["p"])
    err = (res["o"].float() - ref).abs().max().item()
    print(f"{tag} | fwd max-abs err {err:.3e} bound {bound:.3e}")
    if not err < bound:
        failures.append(f"fwd max-abs {err}")
    if c["backward"]:
        ref.backward(t["dout"].float())
        pairs = [("dq", q.grad), ("dk", k.grad), ("dv", v.grad)]
        if table is not None:
            pairs.append(("dtable", table.grad))
        for name, want in pairs:
            got = res[name].float()
            assert torch.isfinite(got).all(), f"{tag}: {name} not finite"
            rel = ((got - want).abs().max() / (want.abs().max() + 1e-6)).item()
            print(f"{tag} | {name} rel err {rel:.3e} bound {GRAD_TOL:.3e}")
            if not rel < GRAD_TOL:
                failures.append(f"{name} rel {rel}")
    assert not failures, f"{tag}: " + ", ".join(failures)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_bits_equal_recorded_build(c):
    _, res = _run(c)
    want = np.load(_TOOL.golden_path(c["name"]))
    names = [n for n in _TOOL.RECORDED if n in res]
    assert sorted(want.files) == sorted(names)
    differing = []
    for name in names:
        got = _TOOL.bits(res[name])
        assert got.shape == want[name].shape and got.dtype == want[name].dtype
        n = int((got != want[name]).sum())
        print(f"[flash-staging] {c['name']} | {name}: {n} of {got.size} words differ")
        if n:
            differing.append(f"{name} ({n} of {got.size})")
    assert not differing, f"{c['name']}: bits differ from the recorded build: " + \
        ", ".join(differing)
