"""Flash forward with a query offset (a chunk of queries behind cached keys):
query row i sits at key position q_offset + i.  Against an fp32 reference,
against the square call (bit for bit) and against the decode kernel."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2  # max abs, forward output vs fp32 (tests/gpu/test_flash_attn_gpu.py)
B, H = 2, 4


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _qkv(sq, sk, d, hkv=H, seed=0):
    torch.manual_seed(seed)
    q = torch.randn(B, sq, H, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, sk, hkv, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, sk, hkv, d, device="cuda", dtype=torch.bfloat16)
    return q, k, v


def _slopes():
    return torch.tensor([2.0 ** -(i + 1) for i in range(H)], device="cuda",
                        dtype=torch.float32)


def _ref(q, k, v, scale, q_offset, kv_len=None, window=0, slopes=None):
    """fp32 [B, Sq, H, D]: query i at position q_offset + i sees key j iff
    j <= q_offset + i, j < kv_len[b], (q_offset + i) - j < window."""
    group = q.shape[2] // k.shape[2]
    qh = q.float().permute(0, 2, 1, 3)
    kh = k.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    vh = v.float().repeat_interleave(group, dim=2).permute(0, 2, 1, 3)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    sq, sk = s.shape[-2:]
    pos = torch.arange(sq, device=q.device)[:, None] + q_offset
    j = torch.arange(sk, device=q.device)[None, :]
    if slopes is not None:
        s = s + slopes[None, :, None, None] * (j - pos).float()[None, None]
    vis = j <= pos
    if window:
        vis = vis & (pos - j < window)
    vis = vis[None, None].expand(q.shape[0], 1, sq, sk)
    if kv_len is not None:
        vis = vis & (j[None, None] < kv_len[:, None, None, None])
    s = s.masked_fill(~vis, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vh).permute(0, 2, 1, 3)


def _check(o, ref, tag):
    err = (o.float() - ref).abs().max().item()
    print(f"[flash-offset] {tag} max abs err {err:.3e}")
    assert err < FWD_TOL, f"{tag}: max abs err {err}"


SHAPES = [(77, 40, 117), (200, 72, 272), (128, 160, 288), (511, 1, 512)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("q_offset,sq,sk", SHAPES)
def test_offset_fwd_matches_reference(d, q_offset, sq, sk):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(sq, sk, d)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, q_offset=q_offset)
    assert o.shape == q.shape
    _check(o, _ref(q, k, v, scale, q_offset), f"d{d} off{q_offset} {sq}x{sk}")


@pytest.mark.parametrize("d", [64, 128])
def test_offset_gqa_matches_reference(d):
    from libai_amd.ops.attention import flash_attention

    q_offset, sq, sk = 200, 72, 272
    q, k, v = _qkv(sq, sk, d, hkv=1)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, q_offset=q_offset)
    _check(o, _ref(q, k, v, scale, q_offset), f"gqa d{d}")


@pytest.mark.parametrize("d", [64, 128])
def test_single_row_matches_reference_and_decode(d):
    from libai_amd.ops.attention import flash_attention, flash_decode_attn

    q, k, v = _qkv(1, 512, d, hkv=1)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, q_offset=511)
        dec = flash_decode_attn(q.permute(0, 2, 1, 3).contiguous(),
                                k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), scale)
    _check(o, _ref(q, k, v, scale, 511), f"one row d{d}")
    _check(o, dec.permute(0, 2, 1, 3).float(), f"one row vs decode d{d}")


@pytest.mark.parametrize("d", [64, 128])
def test_offset_kv_len_matches_reference(d):
    from libai_amd.ops.attention import flash_attention

    q_offset, sq, sk = 200, 72, 320
    q, k, v = _qkv(sq, sk, d)
    kv_len = torch.tensor([272, 250], device="cuda", dtype=torch.int32)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, kv_len=kv_len,
                            q_offset=q_offset)
    _check(o, _ref(q, k, v, scale, q_offset, kv_len=kv_len), f"kv_len d{d}")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("window", [40, 100])
def test_offset_window_matches_reference(d, window):
    from libai_amd.ops.attention import flash_attention

    q_offset, sq, sk = 200, 72, 272
    q, k, v = _qkv(sq, sk, d)
    scale = 1.0 / math.sqrt(d)
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, window=window,
                            q_offset=q_offset)
    _check(o, _ref(q, k, v, scale, q_offset, window=window), f"W{window} d{d}")


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("q_offset,sq,sk", [(77, 40, 117), (128, 160, 288)])
def test_offset_alibi_matches_reference(d, q_offset, sq, sk):
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(sq, sk, d)
    scale = 1.0 / math.sqrt(d)
    slopes = _slopes()
    with torch.no_grad():
        o = flash_attention(q, k, v, scale, causal=True, alibi_slopes=slopes,
                            q_offset=q_offset)
        plain = flash_attention(q, k, v, scale, causal=True, q_offset=q_offset)
    _check(o, _ref(q, k, v, scale, q_offset, slopes=slopes),
           f"alibi d{d} off{q_offset}")
    # the bias must matter at this shape, or the comparison shows nothing
    assert (o.float() - plain.float()).abs().max().item() > FWD_TOL


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("variant", ["plain", "alibi", "window"])
@pytest.mark.parametrize("s,q_offset", [(288, 128), (160, 72)])
def test_chunk_equals_rows_of_the_square_call(d, variant, s, q_offset):
    """A row's key walk and arithmetic are the same in both calls (the tile
    classes compute visible entries alike), block-aligned or not."""
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(s, s, d, seed=1)
    scale = 1.0 / math.sqrt(d)
    kw = {"alibi": dict(alibi_slopes=_slopes()), "window": dict(window=50),
          "plain": {}}[variant]
    with torch.no_grad():
        full = flash_attention(q, k, v, scale, causal=True, **kw)
        chunk = flash_attention(q[:, q_offset:], k, v, scale, causal=True,
                                q_offset=q_offset, **kw)
    assert torch.equal(full[:, q_offset:], chunk)


def test_hidden_keys_have_no_influence():
    """Keys above a row's position, or below its window, never reach it."""
    from libai_amd.ops.attention import flash_attention

    d, q_offset, sq, sk, window = 64, 200, 72, 272, 40
    q, k, v = _qkv(sq, sk, d, seed=2)
    scale = 1.0 / math.sqrt(d)
    row = 10  # position 210: sees keys [0, 210], windowed [171, 210]
    pos = q_offset + row
    k2, v2 = k.clone(), v.clone()
    k2[:, pos + 1:] = 7.0
    v2[:, pos + 1:] = -5.0
    with torch.no_grad():
        a = flash_attention(q, k, v, scale, causal=True, q_offset=q_offset)
        b = flash_attention(q, k2, v2, scale, causal=True, q_offset=q_offset)
    assert torch.equal(a[:, :row + 1], b[:, :row + 1])
    assert not torch.equal(a[:, row + 1:], b[:, row + 1:])
    k3, v3 = k2.clone(), v2.clone()
    k3[:, :pos - window + 1] = 7.0
    v3[:, :pos - window + 1] = -5.0
    with torch.no_grad():
        a = flash_attention(q, k, v, scale, causal=True, window=window,
                            q_offset=q_offset)
        b = flash_attention(q, k3, v3, scale, causal=True, window=window,
                            q_offset=q_offset)
    assert torch.equal(a[:, row], b[:, row])
    assert not torch.equal(a[:, :row], b[:, :row])


def test_zero_offset_keeps_top_left_alignment():
    """q_offset = 0 with Sq != Sk is the call it always was."""
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(72, 272, 64)
    with torch.no_grad():
        a = flash_attention(q, k, v, 0.125, causal=True)
        b = flash_attention(q, k[:, :72], v[:, :72], 0.125, causal=True)
    assert torch.equal(a, b)


def test_binding_rejects_bad_offsets():
    from libai_amd.ops._ext import ext

    q, k, v = _qkv(72, 272, 64)
    f = ext().flash_fwd

    def call(sq=72, causal=True, p=0.0, rel=None, ds=None, de=None, off=200):
        return f(q[:, :sq], k, v, 0.125, p, 1, causal, None, None, 0, rel, ds, de,
                 off)

    call()  # the valid call
    with pytest.raises(RuntimeError, match="causal"):
        call(causal=False)
    with pytest.raises(RuntimeError, match="dropout"):
        call(p=0.1)
    with pytest.raises(RuntimeError, match="rel_bias"):
        call(rel=torch.zeros(H, 72 + 272 - 1, device="cuda"))
    docs = torch.zeros(B, 72, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="document"):
        call(ds=docs, de=docs + 72)
    with pytest.raises(RuntimeError, match="exceed"):
        call(off=201)
    with pytest.raises(RuntimeError, match="q_offset"):
        call(off=-1)


def test_wrapper_refuses_gradients():
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(72, 272, 64)
    q.requires_grad_(True)
    with pytest.raises(ValueError, match="no backward"):
        flash_attention(q, k, v, 0.125, causal=True, q_offset=200)
