"""Tile classes of the flash-attention training kernels.

flash_fwd, flash_bwd_q and flash_bwd_kv sort every 32-row sub-tile into
"interior" (every (q, kv) pair visible: a body without compares or selects) or
"edge" (diagonal, ragged, padded or outside the sliding window: the masked
body).  Each shape here is the smallest that puts skipped, edge and interior
sub-tiles of all three kernels in play; forward and dq/dk/dv are compared with
an fp32 PyTorch reference (tests/dropout_oracle.py, which also supplies the
same-mask reference for dropout).

Bounds are the project's: 2e-2 max-abs forward and 5e-2 of the reference
gradient's max-abs (tests/gpu/test_flash_attn_gpu.py); with dropout the
forward bound is divided by 1 - p (tests/gpu/test_dropout_exact_gpu.py).
Every test prints the error it measured next to its bound before it asserts.
"""

import math

import pytest
import torch

from tests.dropout_oracle import (attn_keep_mask, keep_scale, ref_attention_masked,
                                  ref_attention_probs)

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2
GRAD_TOL = 5e-2
SEED = (1 << 61) + 0xDEADBEEF


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
    print(f"[tile-classes] {tag} | {name} err {err:.3e} bound {bound:.3e}")


def _qkv(b, s, h, d, hkv=None, seed=0):
    torch.manual_seed(seed)
    hkv = hkv or h
    mk = lambda n: torch.randn(b, s, n, d, device="cuda", dtype=torch.bfloat16)
    return mk(h), mk(hkv), mk(hkv)


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


def _fwd_bwd_vs_ref(tag, b, s, h, d, causal, p=0.0, hkv=None, kv_len=None,
                    alibi=False, window=0, seed=0):
    q, k, v = _qkv(b, s, h, d, hkv=hkv, seed=seed)
    scale = 1.0 / math.sqrt(d)
    slopes = _slopes(h) if alibi else None
    tag = f"{tag} d{d} s{s} p{p}"

    o, lse = _ext().flash_fwd(q, k, v, scale, p, SEED, causal, kv_len, slopes, window)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    ref = ref_attention_masked(qr, kr, vr, scale, _keep(b, h, s, p), keep_scale(p),
                               causal, kv_len=kv_len, alibi_slopes=slopes,
                               window=window)
    assert torch.isfinite(o.float()).all(), f"{tag}: forward not finite"
    fwd_bound = FWD_TOL / (1 - p)
    err = (o.float() - ref).abs().max().item()
    _report(tag, "fwd max-abs", err, fwd_bound)

    torch.manual_seed(seed + 100)
    g = torch.randn(b, s, h, d, device="cuda").to(torch.bfloat16)
    if kv_len is not None:
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = torch.arange(s, device="cuda")[None, :] < kv_len[:, None]
        g = g * qmask[:, :, None, None].to(g.dtype)
    dq, dk, dv = _ext().flash_bwd(q, k, v, o, g, lse, scale, p, SEED, causal, None,
                                  kv_len, slopes, window)
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


# 1. causal, S = 192: the second 128-row block is half empty (out-of-range
#    waves); every wave meets skipped, diagonal and interior sub-tiles, over
#    more than one staging round / q tile -------------------------------------
# 2. causal, S = 200: the last q sub-tile and the last kv wave are ragged, so
#    the edge class comes from Sq / Sk rather than from the diagonal ----------
@pytest.mark.parametrize("s", [192, 200])
@pytest.mark.parametrize("d", [64, 128])
def test_causal_matches_reference(d, s):
    _fwd_bwd_vs_ref("causal", 2, s, 2, d, True, seed=1)


# 3. non-causal with kv_len: interior / edge decided by kv_len alone ----------
@pytest.mark.parametrize("d", [64, 128])
def test_kv_len_decides_the_class_and_padded_keys_get_zero_grads(d):
    s = 160
    lens = torch.tensor([160, 97, 32, 1], device="cuda", dtype=torch.int32)
    dk, dv = _fwd_bwd_vs_ref("kv_len", 4, s, 2, d, False, kv_len=lens, seed=2)
    pad = torch.arange(s, device="cuda")[None, :] >= lens[:, None]
    assert dk.float()[pad].abs().max().item() == 0.0, "dK at a padded key"
    assert dv.float()[pad].abs().max().item() == 0.0, "dV at a padded key"


# 4. causal GQA: bwd_kv's group loop re-stages per query head ----------------
@pytest.mark.parametrize("d", [64, 128])
def test_causal_gqa_matches_reference(d):
    _fwd_bwd_vs_ref("gqa 4 on 2", 2, 192, 4, d, True, hkv=2, seed=3)


# 5. causal dropout against the same-mask reference ------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("d", [64, 128])
def test_causal_dropout_matches_same_mask_reference(d, p):
    _fwd_bwd_vs_ref("dropout", 2, 192, 2, d, True, p=p, seed=4)


def _onehot_block(b, s, h, d, c):
    """[B, S, H, D] bf16: row r of block c (c*D <= r < (c+1)*D) holds the
    one-hot vector of r - c*D, every other row is zero."""
    t = torch.zeros(b, s, h, d, device="cuda", dtype=torch.bfloat16)
    r = torch.arange(c * d, min((c + 1) * d, s), device="cuda")
    t[:, r, :, r - c * d] = 1
    return t


def _check_dropped_probs(pd, p_ref, keep, p, tag):
    """pd: the kernel's dropped probabilities [B, H, S, S].  Masked (above the
    diagonal) and dropped entries are exact zeros, kept ones are non-zero
    wherever the fp32 probability is representable and lie within bf16
    rounding of P / (1 - p)."""
    live = p_ref > 1e-30
    wrong = ((pd != 0) != keep) & live
    assert not wrong.any(), (
        f"{tag}: {int(wrong.sum())} entries differ from the oracle mask, first at "
        f"{wrong.nonzero()[0].tolist()}")
    assert (pd[p_ref == 0] == 0).all(), f"{tag}: a masked entry is non-zero"
    assert (pd[~keep] == 0).all(), f"{tag}: a dropped entry is non-zero"
    want = p_ref * float(keep_scale(p))
    sel = live & keep
    err = (pd - want).abs()[sel]
    bound = 2.0 ** -7 * want[sel] + FWD_TOL / (1 - p)
    _report(tag, "Pd max of err / (2^-7 * ref + fwd bound)",
            (err / bound).max().item(), 1.0)
    assert (err <= bound).all(), f"{tag}: kept value off by {err.max().item()}"


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("d", [64, 128])
def test_causal_dropout_masked_and_dropped_probs_are_exact_zeros(d, p):
    """V (or dO) a one-hot block over the key (query) index turns O (dV) into
    a block of the dropped probability matrix, as the forward (the dK/dV
    kernel) regenerates it in its interior and edge bodies."""
    b, h, s = 2, 2, 192
    q, k, v = _qkv(b, s, h, d, seed=5)
    scale = 1.0 / math.sqrt(d)
    p_ref = ref_attention_probs(q, k, scale, True)
    keep = _keep(b, h, s, p)
    nblk = (s + d - 1) // d
    cols = [_ext().flash_fwd(q, k, _onehot_block(b, s, h, d, c), scale, p, SEED, True,
                             None, None, 0)[0] for c in range(nblk)]
    pd = torch.cat(cols, dim=3)[..., :s].permute(0, 2, 1, 3).float()
    _check_dropped_probs(pd, p_ref, keep, p, f"fwd Pd d{d} p{p}")

    o, lse = _ext().flash_fwd(q, k, v, scale, p, SEED, True, None, None, 0)
    rows = [_ext().flash_bwd(q, k, v, o, _onehot_block(b, s, h, d, c), lse, scale, p,
                             SEED, True, None, None, None, 0)[2] for c in range(nblk)]
    pd = torch.cat(rows, dim=3)[..., :s].permute(0, 2, 3, 1).float()
    _check_dropped_probs(pd, p_ref, keep, p, f"dV-path Pd d{d} p{p}")


# 6. ALiBi and sliding window: W = 40 has no band-interior 64-key tile,
#    W = 100 has some ---------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_causal_alibi_matches_reference(d):
    _fwd_bwd_vs_ref("alibi", 2, 192, 2, d, True, alibi=True, seed=6)


@pytest.mark.parametrize("window", [40, 100])
@pytest.mark.parametrize("d", [64, 128])
def test_causal_window_matches_reference(d, window):
    _fwd_bwd_vs_ref(f"window{window}", 2, 192, 2, d, True, window=window, seed=7)


# 7. padding must not change the unpadded rows ------------------------------
def test_zero_padding_leaves_the_first_rows_bit_identical():
    """Causal S = 256, then the same tensors zero-padded to S = 320 with
    kv_len = 256 and the upstream gradient zero beyond row 256: O, dQ, dK and
    dV of the first 256 rows are bit-identical.  Every sub-tile of those rows
    has the same class in both runs (the padding only adds edge tiles that
    contribute exact zeros), so this checks that padded tiles add nothing; the
    test below is the one that moves rows from one body to the other."""
    b, h, d, s, s2 = 2, 2, 64, 256, 320
    q, k, v = _qkv(b, s, h, d, seed=8)
    torch.manual_seed(108)
    g = torch.randn(b, s, h, d, device="cuda").to(torch.bfloat16)
    _padded_run_equals_unpadded(q, k, v, g, s2, causal=True, unpadded_kv_len=False)


def _padded_run_equals_unpadded(q, k, v, g, s2, causal, unpadded_kv_len):
    """Run [B, S, H, D] tensors as they are, then zero-padded to S2 rows with
    kv_len = S and dO zero on the pad; the first S rows of O, lse, dQ, dK and
    dV must be torch.equal."""
    b, s, h, d = q.shape
    scale = 1.0 / math.sqrt(d)
    lens = torch.full((b,), s, device="cuda", dtype=torch.int32)
    l1 = lens if unpadded_kv_len else None
    o, lse = _ext().flash_fwd(q, k, v, scale, 0.0, 0, causal, l1, None, 0)
    dq, dk, dv = _ext().flash_bwd(q, k, v, o, g, lse, scale, 0.0, 0, causal, None, l1,
                                  None, 0)

    def pad(t):
        out = torch.zeros(b, s2, h, d, device="cuda", dtype=t.dtype)
        out[:, :s] = t
        return out

    qp, kp, vp, gp = pad(q), pad(k), pad(v), pad(g)
    o2, lse2 = _ext().flash_fwd(qp, kp, vp, scale, 0.0, 0, causal, lens, None, 0)
    dq2, dk2, dv2 = _ext().flash_bwd(qp, kp, vp, o2, gp, lse2, scale, 0.0, 0, causal,
                                     None, lens, None, 0)
    assert torch.equal(lse, lse2[:, :, :s]), "lse differs between the two runs"
    for name, a, a2 in (("O", o, o2), ("dQ", dq, dq2), ("dK", dk, dk2),
                        ("dV", dv, dv2)):
        diff = (a.float() - a2[:, :s].float()).abs().max().item()
        print(f"[tile-classes] padded vs unpadded d{d} s{s}->{s2} | {name} "
              f"max-abs diff {diff:.3e}")
        assert torch.equal(a, a2[:, :s]), f"{name} differs between the two runs"


# 8. the two bodies compute identical values ---------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_interior_and_edge_bodies_agree_bit_for_bit(d):
    """Non-causal S = 200 against the same tensors zero-padded to S = 224 with
    kv_len = 200 and dO zero on the pad.  Query rows 192..199 sit in a ragged
    (edge) sub-tile in the first run and, against the keys below 192, in an
    interior one in the second: the forward and bwd_q compute their O and dQ,
    and bwd_kv their contribution to every dK and dV row, with the other body.
    The padded queries contribute exact zeros (dO = 0 gives dPd = Drow = 0) and
    keys 200..223 are masked in both runs, so every output of the first 200
    rows is bit-identical iff both bodies compute visible entries alike."""
    b, h, s, s2 = 2, 2, 200, 224
    q, k, v = _qkv(b, s, h, d, seed=9)
    torch.manual_seed(109)
    g = torch.randn(b, s, h, d, device="cuda").to(torch.bfloat16)
    _padded_run_equals_unpadded(q, k, v, g, s2, causal=False, unpadded_kv_len=False)
