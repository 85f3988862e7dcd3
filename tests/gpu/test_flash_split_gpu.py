"""Split-KV flash forward (``flash_attention(..., kv_split=n)``): a short query
chunk behind a long cache, the query heads of a KV head packed into one tile,
the keys cut into splits whose partial states a merge kernel folds.  Against a
plain fp32 reference, output and logsumexp."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2   # max abs, forward output vs fp32 (tests/gpu/test_flash_offset_gpu.py)
# max abs, logsumexp vs fp32: twice what the single-pass kernel (_C.flash_fwd)
# shows at the shapes below, 2.842e-3 (worst: d 64, 256 x 256 causal; the
# bf16 rounding of the pre-scaled Q), rounded down.  The split path measured
# the same.
LSE_TOL = 5.68e-3
LAYER_TOL = 3e-2  # flash vs unfused layer output, relative (test_prefill_flash_gpu.py)
B, H = 2, 4


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _qkv(sq, sk, d, hkv):
    torch.manual_seed(0)
    q = torch.randn(B, sq, H, d, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, sk, hkv, d, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, sk, hkv, d, device="cuda", dtype=torch.bfloat16)
    return q, k, v


def _ref(q, k, v, scale, q_offset, causal=True, kv_len=None, window=0, slopes=None):
    """fp32 (o [B, Sq, H, D], lse [B, H, Sq]): query i at position q_offset + i
    sees key j iff j < kv_len[b], and under causal j <= q_offset + i and
    (q_offset + i) - j < window."""
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
    vis = (j <= pos) if causal else torch.ones(sq, sk, dtype=torch.bool, device=q.device)
    if window:
        vis = vis & (pos - j < window)
    vis = vis[None, None].expand(q.shape[0], 1, sq, sk)
    if kv_len is not None:
        vis = vis & (j[None, None] < kv_len[:, None, None, None])
    s = s.masked_fill(~vis, float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), vh).permute(0, 2, 1, 3)
    return o, torch.logsumexp(s, dim=-1)


def _run_and_check(tag, d, q_offset, sq, sk, hkv, split_keys=128, causal=True,
                   kv_len=None, window=0, slopes=None, check_lse=True):
    from libai_amd.ops._ext import ext
    from libai_amd.ops.attention import flash_attention

    q, k, v = _qkv(sq, sk, d, hkv)
    scale = 1.0 / math.sqrt(d)
    if check_lse:
        o, lse = ext().flash_fwd_split(q, k, v, scale, causal, kv_len, slopes, window,
                                       q_offset, split_keys)
    else:  # the public call returns o alone
        with torch.no_grad():
            o = flash_attention(q, k, v, scale, causal=causal, kv_len=kv_len,
                                alibi_slopes=slopes, window=window, q_offset=q_offset,
                                kv_split=split_keys)
    ro, rlse = _ref(q, k, v, scale, q_offset, causal, kv_len, window, slopes)
    err = (o.float() - ro).abs().max().item()
    print(f"[flash-split] {tag} d{d} o max abs err {err:.3e}")
    assert o.shape == q.shape and err < FWD_TOL, f"{tag}: o max abs err {err}"
    if check_lse:
        lerr = (lse - rlse).abs().max().item()
        print(f"[flash-split] {tag} d{d} lse max abs err {lerr:.3e}")
        assert lse.shape == rlse.shape and lerr < LSE_TOL, f"{tag}: lse err {lerr}"


# (q_offset, sq, sk, hkv, split_keys)
CAUSAL = [
    (200, 72, 272, 4, 128),  # G=1, ragged 16-key last split, diagonal across a split
    (376, 8, 384, 1, 128),   # G=4: 32 packed rows, one wave holding four heads
    (256, 5, 261, 1, 128),   # 20 packed rows, heads wrap at 5, a 5-key last split
    (156, 100, 256, 2, 128),  # 200 rows in two tiles, a wave across the head boundary
    (0, 256, 256, 4, 128),   # null second split for rows 0..127, interior sub-tiles
    (511, 1, 512, 1, 128),   # one token
    (200, 72, 272, 4, 256),
]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("q_offset,sq,sk,hkv,split_keys", CAUSAL)
def test_split_causal_matches_reference(d, q_offset, sq, sk, hkv, split_keys):
    _run_and_check(f"off{q_offset} {sq}x{sk} hkv{hkv} split{split_keys}", d, q_offset,
                   sq, sk, hkv, split_keys)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal,q_offset,sq,sk,lens",
                         [(True, 200, 72, 272, (272, 130)),
                          (False, 0, 40, 328, (328, 200))])
def test_split_kv_len_matches_reference(d, causal, q_offset, sq, sk, lens):
    """Batch 1 of the causal case: a 2-key second split, a null third split
    and positions beyond its keys."""
    kv_len = torch.tensor(lens, device="cuda", dtype=torch.int32)
    _run_and_check(f"kv_len causal={causal}", d, q_offset, sq, sk, 1, causal=causal,
                   kv_len=kv_len)


@pytest.mark.parametrize("d", [64, 128])
def test_split_alibi_takes_each_lanes_own_slope(d):
    slopes = torch.tensor([2.0 ** -(i + 1) for i in range(H)], device="cuda",
                          dtype=torch.float32)
    _run_and_check("alibi", d, 376, 8, 384, 1, slopes=slopes)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("window", [40, 150])
@pytest.mark.parametrize("q_offset,sq,sk,hkv", [(200, 72, 272, 4), (376, 8, 384, 1)])
def test_split_window_matches_reference(d, window, q_offset, sq, sk, hkv):
    """Splits entirely below the band and a band border inside a split."""
    _run_and_check(f"window{window} {sq}x{sk} hkv{hkv}", d, q_offset, sq, sk, hkv,
                   window=window, check_lse=False)


@pytest.mark.parametrize("kind,kvh", [("llama", 1), ("mha", 4)])
def test_layer_split_route_matches_flag_off(kind, kvh):
    """A 16-token chunk on 2048 cached keys, 4 heads (LlamaAttention on 1 KV
    head, MultiheadAttention): too few workgroups for flash_chunk_pays, so
    flash_prefill=True keeps the materialized route (bit-equal to flag off)
    and "split" takes the split-KV forward.  The flag-off Llama layer does not
    mask among the tokens of a chunk (on this input its chunk call is 0.26
    relative away from its own token-by-token steps, fp32 on the CPU), so the
    flag-off reference for every row is the layer fed the 16 tokens one at a
    time; its chunk call is the reference for the cache and for the last row,
    which sees every key either way."""
    from libai_amd.layers import MultiheadAttention
    from libai_amd.models.llama import LlamaAttention
    from libai_amd.ops.attention import flash_chunk_pays, flash_split_keys

    past_len, step = 2048, 16
    assert not flash_chunk_pays(1, 4, step, past_len + step)
    assert flash_split_keys(1, kvh, 4 // kvh, step, past_len + step) > 0
    init = torch.nn.init.xavier_normal_

    def make(flag):
        if kind == "llama":
            return LlamaAttention(256, 4, 4096, init, init, num_key_value_heads=kvh,
                                  flash_prefill=flag)
        return MultiheadAttention(256, 4, attn_mask_type="causal", flash_prefill=flag)

    torch.manual_seed(1)
    off = make(False).to("cuda", torch.bfloat16).eval()
    on = make("split").to("cuda", torch.bfloat16).eval()
    on.load_state_dict(off.state_dict())
    past = tuple(torch.randn(1, kvh, past_len, 64, device="cuda", dtype=torch.bfloat16)
                 for _ in range(2))
    x = torch.randn(1, step, 256, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        y0, c0 = off(x, past_key_value=past, use_cache=True)
        y1, c1 = on(x, past_key_value=past, use_cache=True)
        rows, cache = [], past
        for t in range(step):
            y, cache = off(x[:, t:t + 1], past_key_value=cache, use_cache=True)
            rows.append(y)
        y_steps = torch.cat(rows, dim=1)
    for a, b in zip(c0, c1):
        assert torch.equal(a, b)
    assert not torch.equal(y0, y1)  # the materialized route would be bit-equal

    def rel_err(got, want):
        return ((got.float() - want.float()).abs().max() / want.float().abs().max()).item()

    rel, rel_last = rel_err(y1, y_steps), rel_err(y1[:, -1], y0[:, -1])
    print(f"[flash-split] {kind} layer rel err vs steps {rel:.3e}, last row vs chunk "
          f"{rel_last:.3e}")
    assert rel < LAYER_TOL, rel
    assert rel_last < LAYER_TOL, rel_last
