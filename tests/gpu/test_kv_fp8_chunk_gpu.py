"""Multi-token steps on the FP8 KV cache: the T-token insert, flash_chunk_fp8
against fp64 and against single-token calls, and greedy speculative
verification on the continuous Llama decoder."""
import functools

import pytest
import torch

from tests.gpu.test_kv_fp8_gpu import FWD_TOL, _quantize, _setup, _tiny_llama  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 1536
HDS = [64, 128]


def _kv_len(t):
    # an empty past, a chunk across a 32-key tile edge, a chunk across the 512
    # split edge (null splits for its lower tokens), three splits
    return [t, 33, 515, 1300]


@pytest.mark.parametrize("hd", HDS)
def test_insert_chunk_equals_steps(hd):
    from libai_amd.ops._ext import ext
    from libai_amd.ops.rope import _tables

    B, T, NH, KVH, MAX = 3, 3, 8, 2, 40
    g = torch.Generator(device=DEV).manual_seed(hd)
    q, k, v = (torch.randn(B, T, h, hd, device=DEV, generator=g).bfloat16()
               for h in (NH, KVH, KVH))
    cos_t, sin_t = _tables(MAX, hd, 10000.0, torch.device(DEV))
    pos = torch.tensor([0, MAX - 2, MAX], device=DEV)
    k8 = torch.randint(0, 256, (B, KVH, MAX, hd), device=DEV, generator=g,
                       dtype=torch.uint8)
    ks = torch.rand(B, KVH, MAX, device=DEV, generator=g) + 0.5
    before = [k8, k8.flip(-1).contiguous(), ks, ks + 1.0]
    one, steps = ([t.clone() for t in before] for _ in range(2))

    qo = ext().rope_kv_insert_fp8(q, k, v, *one, cos_t, sin_t, pos, True)
    assert qo.shape == (B, NH, T, hd)
    written = torch.zeros(B, KVH, MAX, dtype=torch.bool, device=DEV)
    for t in range(T):
        qo_t = ext().rope_kv_insert_fp8(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1],
                                        *steps, cos_t, sin_t, pos + t, True)
        for b in range(B):
            if int(pos[b]) + t < MAX:  # out-of-range rows are skipped one by one
                written[b, :, int(pos[b]) + t] = True
                assert torch.equal(qo[b, :, t], qo_t[b, :, 0])
    assert int(written.sum()) == 5 * KVH
    for got, ref, old in zip(one, steps, before):
        assert torch.equal(got, ref)
        assert torch.equal(got[~written], old[~written])
        assert not torch.equal(got[written], old[written])


@functools.lru_cache(maxsize=None)
def _case(hd, group, t, cap=CAP, b=4):
    """As test_kv_fp8_gpu._case, with T queries; the last T keys of the longest
    row carry the largest V scale, so each of them alone (window=1) is far from
    its token's average over ~1300 keys."""
    gen = torch.Generator(device=DEV).manual_seed(1000 * hd + 10 * group + t)
    kvh, n = 2, _kv_len(t)[-1]
    q = torch.randn(b, kvh * group, t, hd, device=DEV, generator=gen).bfloat16()
    k8, ks, kd = _quantize(torch.randn(b, kvh, cap, hd, device=DEV, generator=gen), gen)
    v8, vs, vd = _quantize(torch.randn(b, kvh, cap, hd, device=DEV, generator=gen), gen,
                           top_row=(b - 1, slice(None), slice(n - t, n)) if b == 4 else None)
    return q, k8, v8, ks * 2.0 ** -3, vs * 2.0 ** -5, kd * 2.0 ** -3, vd * 2.0 ** -5


def _reference(q, kd, vd, kv_len, window, scale):
    """fp64 softmax attention over the dequantized cache: token t at position
    p = n - T + t sees the keys j <= p with p - j < window."""
    b, h, t, d = q.shape
    kvh = kd.shape[1]
    out = torch.empty(b, h, t, d, dtype=torch.float64, device=q.device)
    for i, n in enumerate(kv_len):
        p = torch.arange(n - t, n, device=q.device)[:, None]
        j = torch.arange(n, device=q.device)[None, :]
        hidden = (j > p) if window is None else (j > p) | (p - j >= window)
        qi = q[i].double().view(kvh, h // kvh, t, d)
        s = qi @ kd[i, :, None, :n].transpose(-1, -2) * scale
        prob = torch.softmax(s.masked_fill(hidden, float("-inf")), dim=-1)
        out[i] = (prob @ vd[i, :, None, :n]).view(h, t, d)
    return out


@pytest.mark.parametrize("window", [None, 1, 3, 513])
@pytest.mark.parametrize("group, t", [(4, 2), (4, 8), (4, 9), (7, 5), (1, 32), (8, 4)])
@pytest.mark.parametrize("hd", HDS)
def test_chunk_against_fp64(hd, group, t, window):
    from libai_amd.ops.attention import flash_decode_attn_fp8

    q, k8, v8, ks, vs, kd, vd = _case(hd, group, t)
    scale = hd ** -0.5
    kv_len = torch.tensor(_kv_len(t), dtype=torch.int32, device=DEV)
    out = flash_decode_attn_fp8(q, k8, v8, ks, vs, scale, kv_len=kv_len,
                                window=window)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    ref = _reference(q, kd, vd, _kv_len(t), window, scale)
    err = (out.double() - ref).abs().amax(dim=(1, 2, 3))
    print(f"hd{hd} g{group} T{t} w{window}: max-abs err per batch {err.tolist()}")
    assert float(err.max()) < FWD_TOL
    if window == 1:  # the window is applied per token: none is its full row
        full = _reference(q, kd, vd, _kv_len(t), None, scale)
        off = (out[3].double() - full[3]).abs().amax(dim=(0, 2))  # per token
        assert float(off.min()) > FWD_TOL


@pytest.mark.parametrize("window", [None, 3])
@pytest.mark.parametrize("group, t", [(4, 9), (7, 5)])
@pytest.mark.parametrize("hd", HDS)
def test_chunk_equals_steps(hd, group, t, window):
    from libai_amd.ops.attention import flash_decode_attn_fp8

    q, k8, v8, ks, vs, _, _ = _case(hd, group, t)
    kv_len = torch.tensor(_kv_len(t), dtype=torch.int32, device=DEV)
    out = flash_decode_attn_fp8(q, k8, v8, ks, vs, hd ** -0.5, kv_len=kv_len,
                                window=window)
    for i in range(t):
        step = flash_decode_attn_fp8(q[:, :, i:i + 1], k8, v8, ks, vs, hd ** -0.5,
                                     kv_len=kv_len - (t - 1 - i), window=window)
        assert torch.equal(out[:, :, i:i + 1], step), f"token {i}"


@pytest.mark.parametrize("hd", HDS)
def test_chunk_capacity_independent(hd):
    from libai_amd.ops.attention import flash_decode_attn_fp8

    q, k8, v8, ks, vs, _, _ = _case(hd, 4, 5, cap=512, b=2)
    kv_len = torch.full((2,), 450, dtype=torch.int32, device=DEV)
    outs = []
    for cap in (512, 1536):
        gen = torch.Generator(device=DEV).manual_seed(cap)
        c8 = [torch.randint(0, 256, (2, 2, cap, hd), device=DEV, generator=gen,
                            dtype=torch.uint8) for _ in range(2)]
        sc = [torch.full((2, 2, cap), float("nan"), device=DEV) for _ in range(2)]
        for dst, src in zip(c8 + sc, (k8, v8, ks, vs)):
            dst[:, :, :450] = src[:, :, :450]
        outs.append(flash_decode_attn_fp8(q, c8[0], c8[1], sc[0], sc[1], hd ** -0.5,
                                          kv_len=kv_len))
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])


@torch.no_grad()
def test_speculate_llama_fp8():
    """Drafts cut from the plain greedy stream: all right, right-right-wrong,
    first wrong.  Measured on MI355X with this seed: logits of the K + 1-token
    step against teacher-forced single steps differ by 0.0000 max-abs, the
    smallest top-2 margin of the compared steps is 0.0078."""
    from libai_amd.inference.captured_decode import ContinuousLlamaDecoder

    model = _tiny_llama()
    gen = torch.Generator(device=DEV).manual_seed(7)
    prompts = [torch.randint(0, 1024, (n,), device=DEV, generator=gen)
               for n in (25, 11, 18)]

    def admitted(**kw):
        dec = ContinuousLlamaDecoder(model, max_batch=3, max_seq_len=64, **kw)
        for slot, p in enumerate(prompts):
            dec.add_request(slot, p)
        return dec

    plain = admitted(kv_cache_dtype="fp8")
    plain.step(11)
    ref = torch.stack([plain.tokens(s) for s in range(3)])  # [3, 12]

    wrong = (ref + 1) % 1024
    draft = ref[:, 1:4].clone()
    draft[1, 2] = wrong[1, 3]
    draft[2, 0] = wrong[2, 1]
    dec = admitted(kv_cache_dtype="fp8")
    logits = dec._speculate_logits(draft).float()  # what speculate() scores

    forced = admitted(kv_cache_dtype="fp8")  # the same tokens, one per step
    diff, margin = 0.0, float("inf")
    for i, tok in enumerate(torch.cat([ref[:, :1], draft], dim=1).unbind(1)):
        forced.static_tok.copy_(tok[:, None])
        single = forced._logits()[:, 0].float()
        diff = max(diff, float((logits[:, i] - single).abs().max()))
        top2 = single.topk(2, dim=-1).values
        margin = min(margin, float((top2[:, 0] - top2[:, 1]).min()))
        forced.pos.add_(1)
        forced.kv32.add_(1)
    print(f"speculate: logits max-abs diff {diff:.4f}, min top-2 margin {margin:.4f}")
    assert diff < FWD_TOL

    n = dec.speculate(draft)
    assert n.tolist() == [3, 2, 0]
    for slot, keep in enumerate((5, 4, 2)):  # the first token, n drafts, the next
        assert torch.equal(dec.tokens(slot), ref[slot, :keep])
    dec.step(3)
    for slot, keep in enumerate((8, 7, 5)):
        assert torch.equal(dec.tokens(slot), ref[slot, :keep])

    with pytest.raises(NotImplementedError):
        admitted().speculate(draft)  # a bf16 cache has no multi-token step
