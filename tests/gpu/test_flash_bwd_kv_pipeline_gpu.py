"""Software-pipelined q-tile loop of flash_bwd_kv at D = 64.

The dK/dV kernel walks 64-row q tiles.  At D = 64 it prefetches tile qt + 1
into registers while it computes tile qt and stores it to LDS afterwards,
between two barriers; the first tile of every (kv block, query head) is staged
directly and the pipeline restarts per GQA query head.  All three training
kernels also rotate the tile a workgroup takes by its head index.  The shapes
here are the smallest at which that can go wrong: one, two and three tiles
(prologue only, one prefetch, a prefetch issued while a prefetched tile is
computed; with a second LDS buffer also the buffer parity), a ragged last tile
(clamped prefetch), a fully padded kv block (no tile at all), a head boundary,
and a sliding window that starts the loop late and ends it early.

Bounds are the project's: 2e-2 max-abs forward and 5e-2 of the reference
gradient's max-abs (tests/gpu/test_flash_attn_gpu.py); with dropout the
forward bound is divided by 1 - p (tests/gpu/test_dropout_exact_gpu.py).  The
reference is fp32 PyTorch with the oracle's dropout mask
(tests/dropout_oracle.py).  Every test prints the error next to its bound
before it asserts.
"""

import math

import pytest
import torch

from tests.dropout_oracle import attn_keep_mask, keep_scale, ref_attention_masked

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2
GRAD_TOL = 5e-2
SEED = (1 << 61) + 0xDEADBEEF
D = 64


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    from libai_amd.ops._ext import has_ext

    assert has_ext(), "HIP extension must be built+loaded on the GPU box"
    yield


def _ext():
    from libai_amd.ops._ext import ext

    return ext()


def _report(tag, name, err, bound):
    print(f"[bwd-kv-pipeline] {tag} | {name} err {err:.3e} bound {bound:.3e}")


def _qkv(b, s, h, hkv=None, seed=0):
    torch.manual_seed(seed)
    hkv = hkv or h
    mk = lambda n: torch.randn(b, s, n, D, device="cuda", dtype=torch.bfloat16)
    return mk(h), mk(hkv), mk(hkv)


def _dout(b, s, h, seed, kv_len=None):
    torch.manual_seed(seed + 100)
    g = torch.randn(b, s, h, D, device="cuda").to(torch.bfloat16)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = torch.arange(s, device="cuda")[None, :] < kv_len[:, None]
        g = g * qmask[:, :, None, None].to(g.dtype)
    return g


_KEEP = {}


def _keep(b, h, s, p):
    """Oracle keep mask [B, H, S, S] on the device (all ones at p = 0);
    computed once per key, read-only."""
    key = (b, h, s, p)
    if key not in _KEEP:
        if p > 0:
            m = attn_keep_mask(SEED, b * h, s, s, p).view(b, h, s, s).cuda()
        else:
            m = torch.ones(b, h, s, s, dtype=torch.bool, device="cuda")
        _KEEP[key] = m
    return _KEEP[key]


def _slopes(h):
    from libai_amd.layers.position_bias import alibi_slopes

    return alibi_slopes(h).to(device="cuda", dtype=torch.float32).contiguous()


def _ref_rel_bias(q, k, v, scale, causal, table):
    """fp32 reference with the [H, 2S - 1] table materialised:
    bias[h, i, j] = table[h, j - i + S - 1]."""
    qh, kh, vh = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    n = s.shape[-1]
    i = torch.arange(n, device=q.device)[:, None]
    j = torch.arange(n, device=q.device)[None, :]
    s = s + table[:, j - i + (n - 1)][None]
    if causal:
        s = s.masked_fill(j > i, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vh).permute(0, 2, 1, 3)


def _fwd_bwd_vs_ref(tag, b, s, h, causal, p=0.0, hkv=None, kv_len=None, alibi=False,
                    window=0, rel_bias=False, seed=0):
    q, k, v = _qkv(b, s, h, hkv=hkv, seed=seed)
    scale = 1.0 / math.sqrt(D)
    slopes = _slopes(h) if alibi else None
    table = None
    if rel_bias:
        gen = torch.Generator(device="cuda").manual_seed(seed + 11)
        table = torch.randn(h, 2 * s - 1, device="cuda", dtype=torch.float32,
                            generator=gen) * 0.5
    tag = f"{tag} s{s} p{p}"

    o, lse = _ext().flash_fwd(q, k, v, scale, p, SEED, causal, kv_len, slopes, window,
                              table)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    if rel_bias:
        ref = _ref_rel_bias(qr, kr, vr, scale, causal, table)
    else:
        ref = ref_attention_masked(qr, kr, vr, scale, _keep(b, h, s, p), keep_scale(p),
                                   causal, kv_len=kv_len, alibi_slopes=slopes,
                                   window=window)
    assert torch.isfinite(o.float()).all(), f"{tag}: forward not finite"
    fwd_bound = FWD_TOL / (1 - p)
    err = (o.float() - ref).abs().max().item()
    _report(tag, "fwd max-abs", err, fwd_bound)

    g = _dout(b, s, h, seed, kv_len)
    dq, dk, dv = _ext().flash_bwd(q, k, v, o, g, lse, scale, p, SEED, causal, None,
                                  kv_len, slopes, window, table)[:3]
    ref.backward(g.float())
    failures = []
    if not err < fwd_bound:
        failures.append(f"fwd max-abs {err}")
    for name, got, want in (("dq", dq, qr.grad), ("dk", dk, kr.grad),
                            ("dv", dv, vr.grad)):
        assert torch.isfinite(got.float()).all(), f"{tag}: {name} not finite"
        rel = ((got.float() - want).abs().max() / (want.abs().max() + 1e-6)).item()
        _report(tag, f"{name} rel", rel, GRAD_TOL)
        if not rel < GRAD_TOL:
            failures.append(f"{name} rel {rel}")
    assert not failures, f"{tag}: " + ", ".join(failures)
    return dk, dv


# 1. causal, one / two / three q tiles: prologue only, one prefetch, two
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("s", [64, 128, 192])
def test_causal_tile_counts_match_reference(s, p):
    _fwd_bwd_vs_ref("causal", 2, s, 2, True, p=p, seed=1)


# 2. ragged: the last tile's prefetch clamps rows >= Sq
def test_ragged_last_tile_matches_reference():
    _fwd_bwd_vs_ref("ragged", 2, 200, 2, True, seed=2)


# 3. batch 1's second kv block (keys 128..255) is fully padded: n_qtiles == 0
def test_fully_padded_kv_block_gets_exact_zeros():
    s = 256
    lens = torch.tensor([256, 40], device="cuda", dtype=torch.int32)
    dk, dv = _fwd_bwd_vs_ref("kv_len", 2, s, 2, False, kv_len=lens, seed=3)
    pad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert dk.float()[pad].abs().max().item() == 0.0, "dK at a padded key"
    assert dv.float()[pad].abs().max().item() == 0.0, "dV at a padded key"


# 4. GQA: the pipeline drains and restarts at each query-head boundary
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gqa_head_boundary_matches_reference(p):
    _fwd_bwd_vs_ref("gqa 4 on 2", 2, 192, 4, True, p=p, hkv=2, seed=4)


# 5. window: kv block 0 ends its loop early (tiles 0..2 of 4), kv block 1
#    starts at qt_start = 2
def test_window_starts_late_and_ends_early():
    _fwd_bwd_vs_ref("window40", 2, 256, 2, True, window=40, seed=5)


# 6. the other D = 64 instantiations
def test_alibi_matches_reference():
    _fwd_bwd_vs_ref("alibi", 2, 192, 2, True, alibi=True, seed=6)


@pytest.mark.parametrize("causal", [True, False])
def test_rel_bias_matches_reference(causal):
    _fwd_bwd_vs_ref(f"relb causal={causal}", 2, 192, 2, causal, rel_bias=True, seed=7)


# 7. tile-count independence, exact
def test_three_and_four_tiles_give_the_same_bits():
    """Non-causal S = 192 (three q tiles), then the same tensors zero-padded
    to S = 256 with kv_len = 192 and dO zero on the pad (four tiles, the last
    one contributing exact zeros): dK and dV of keys 0..191 and dQ of rows
    0..191 are bit-equal."""
    b, h, s, s2 = 2, 2, 192, 256
    q, k, v = _qkv(b, s, h, seed=8)
    g = _dout(b, s, h, 8)
    scale = 1.0 / math.sqrt(D)
    lens = torch.full((b,), s, device="cuda", dtype=torch.int32)
    o, lse = _ext().flash_fwd(q, k, v, scale, 0.0, 0, False, None, None, 0)
    dq, dk, dv = _ext().flash_bwd(q, k, v, o, g, lse, scale, 0.0, 0, False, None, None,
                                  None, 0)

    def pad(t):
        out = torch.zeros(b, s2, h, D, device="cuda", dtype=t.dtype)
        out[:, :s] = t
        return out

    qp, kp, vp, gp = pad(q), pad(k), pad(v), pad(g)
    o2, lse2 = _ext().flash_fwd(qp, kp, vp, scale, 0.0, 0, False, lens, None, 0)
    dq2, dk2, dv2 = _ext().flash_bwd(qp, kp, vp, o2, gp, lse2, scale, 0.0, 0, False,
                                     None, lens, None, 0)
    for name, a, a2 in (("dQ", dq, dq2), ("dK", dk, dk2), ("dV", dv, dv2)):
        diff = (a.float() - a2[:, :s].float()).abs().max().item()
        print(f"[bwd-kv-pipeline] 3 vs 4 tiles | {name} max-abs diff {diff:.3e}")
        assert torch.equal(a, a2[:, :s]), f"{name} differs between 3 and 4 tiles"


# 8. no atomics in dK/dV: two calls differ only if a buffer is raced on
@pytest.mark.parametrize("hkv", [4, 2])
def test_two_backward_calls_are_bit_equal(hkv):
    b, h, s, p = 2, 4, 192, 0.1
    q, k, v = _qkv(b, s, h, hkv=hkv, seed=9)
    g = _dout(b, s, h, 9)
    scale = 1.0 / math.sqrt(D)
    o, lse = _ext().flash_fwd(q, k, v, scale, p, SEED, True, None, None, 0)
    runs = [_ext().flash_bwd(q, k, v, o, g, lse, scale, p, SEED, True, None, None,
                             None, 0) for _ in range(2)]
    for name, i in (("dK", 1), ("dV", 2)):
        diff = (runs[0][i].float() - runs[1][i].float()).abs().max().item()
        print(f"[bwd-kv-pipeline] repeat hkv{hkv} | {name} max-abs diff {diff:.3e}")
        assert torch.equal(runs[0][i], runs[1][i]), f"{name} differs between two calls"
