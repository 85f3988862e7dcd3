"""FP8 (e4m3) KV cache: quantizing insert, prefill row quantizer, packed-GQA
MFMA decode kernel and the captured / continuous Llama decoders on it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2  # max-abs (the project's bound for bf16 outputs)
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _e4m3(c8):
    return c8.view(torch.float8_e4m3fn).float()


def _check_quantized(c8_rows, scale_rows, ref_rows, tag):
    """c8_rows [..., HD] uint8 and scale_rows [...] against the bf16 rows they
    quantize.  e4m3 keeps 3 mantissa bits (half an ulp = 2^-4 relative) and its
    subnormals are 2^-9 apart."""
    ref = ref_rows.float()
    amax = ref.abs().amax(-1)
    torch.testing.assert_close(scale_rows, amax / 448.0, rtol=1e-6, atol=0)
    code = _e4m3(c8_rows)
    err = (code * scale_rows[..., None] - ref).abs()
    bound = ref.abs() * 2.0 ** -4 + scale_rows[..., None] * 2.0 ** -10
    assert bool((err <= bound).all()), f"{tag}: worst excess {(err - bound).max()}"
    top = code.gather(-1, ref.abs().argmax(-1, keepdim=True)).abs()
    assert bool((top == 448.0).all()), f"{tag}: the row maximum must decode to 448"


@pytest.mark.parametrize("rot", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
def test_insert(hd, rot):
    from libai_amd.ops._ext import ext
    from libai_amd.ops.rope import _tables

    B, NH, KVH, MAX = 3, 8, 2, 40
    g = torch.Generator(device=DEV).manual_seed(hd + rot)
    q, k, v = (torch.randn(B, 1, h, hd, device=DEV, generator=g).bfloat16()
               for h in (NH, KVH, KVH))
    k = k * 3.0
    cos_t, sin_t = _tables(MAX, hd, 10000.0, torch.device(DEV))
    pos = torch.tensor([0, 39, 40], device=DEV)
    ck = torch.randn(B, KVH, MAX, hd, device=DEV, generator=g).bfloat16()
    cv = ck.clone()
    k8 = torch.randint(0, 256, (B, KVH, MAX, hd), device=DEV, generator=g,
                       dtype=torch.uint8)
    v8 = k8.flip(-1).contiguous()
    ks = torch.rand(B, KVH, MAX, device=DEV, generator=g) + 0.5
    vs = ks + 1.0
    before = [t.clone() for t in (k8, v8, ks, vs)]

    qo_ref = ext().rope_kv_insert(q, k, v, ck, cv, cos_t, sin_t, pos, rot)
    qo = ext().rope_kv_insert_fp8(q, k, v, k8, v8, ks, vs, cos_t, sin_t, pos, rot)
    # both kernels skip the out-of-range batch whole: its qo rows are unwritten
    assert torch.equal(qo[:2], qo_ref[:2])
    written = torch.zeros(B, KVH, MAX, dtype=torch.bool, device=DEV)
    for b in (0, 1):
        p = int(pos[b])
        written[b, :, p] = True
        _check_quantized(k8[b, :, p], ks[b, :, p], ck[b, :, p], f"k b{b}")
        _check_quantized(v8[b, :, p], vs[b, :, p], cv[b, :, p], f"v b{b}")
    # the out-of-range batch and every other row keep their bytes and scales
    for got, old in zip((k8, v8, ks, vs), before):
        assert torch.equal(got[~written], old[~written])


@pytest.mark.parametrize("hd", [64, 128])
def test_quantize_rows_strided(hd):
    from libai_amd.ops.kv_cache import alloc_fp8_cache, quantize_rows

    g = torch.Generator(device=DEV).manual_seed(hd)
    src = (torch.randn(2, 37, 2, hd, device=DEV, generator=g) * 2.0).bfloat16()
    src = src.permute(0, 2, 1, 3)  # [2, 2, 37, hd], strided
    src[1, 0, 5] = 0  # an all-zero row takes scale 1
    c8, sc = alloc_fp8_cache(2, 2, 40, hd, DEV)
    c8.fill_(7)
    sc.fill_(3.0)
    quantize_rows(src, c8, sc)
    assert float(sc[1, 0, 5]) == 1.0 and int(c8[1, 0, 5].max()) == 0
    keep = torch.ones(2, 2, 37, dtype=torch.bool, device=DEV)
    keep[1, 0, 5] = False
    _check_quantized(c8[:, :, :37][keep], sc[:, :, :37][keep], src[keep], "rows")
    assert bool((c8[:, :, 37:] == 7).all()) and bool((sc[:, :, 37:] == 3.0).all())


# ---- decode ---------------------------------------------------------------
KV_LEN = [1, 65, 512, 1300]  # one key, a tile edge, a split edge, three splits
CAP = 1536


def _quantize(x, gen, top_row=None):
    """Rows of x rescaled to amax 2^u, u uniform in [-6, 6] (6 for top_row),
    then quantized by the cache's rule -> (bytes, scale, fp64 dequantized
    values)."""
    u = torch.rand(x.shape[:-1], device=DEV, generator=gen) * 12.0 - 6.0
    if top_row is not None:
        u[top_row] = 6.0
    x = x / x.abs().amax(-1, keepdim=True) * torch.exp2(u)[..., None]
    scale = x.abs().amax(-1) / 448.0
    c8 = (x / scale[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return c8.view(torch.uint8), scale, c8.float().double() * scale[..., None].double()


@functools.lru_cache(maxsize=None)
def _case(hd, group, cap=CAP, b=4):
    """Inputs shared by the window cases.  The scales spread over 2^+-6 around
    2^-3 / 448 (K) and 2^-5 / 448 (V), so scores and outputs stay O(1) and
    FWD_TOL is the bound of bf16 outputs of that size.  The last key of the
    longest row has the largest V scale: alone under window=1 it is far from
    the average over all 1300 keys."""
    gen = torch.Generator(device=DEV).manual_seed(1000 * hd + group)
    kvh = 2
    q = torch.randn(b, kvh * group, 1, hd, device=DEV, generator=gen).bfloat16()
    k8, ks, kd = _quantize(torch.randn(b, kvh, cap, hd, device=DEV, generator=gen), gen)
    v8, vs, vd = _quantize(torch.randn(b, kvh, cap, hd, device=DEV, generator=gen), gen,
                           top_row=(b - 1, slice(None), KV_LEN[-1] - 1) if b == 4 else None)
    return q, k8, v8, ks * 2.0 ** -3, vs * 2.0 ** -5, kd * 2.0 ** -3, vd * 2.0 ** -5


def _reference(q, kd, vd, kv_len, window, scale):
    """fp64 softmax attention over the dequantized cache."""
    b, h, _, d = q.shape
    kvh = kd.shape[1]
    out = torch.empty(b, h, 1, d, dtype=torch.float64, device=q.device)
    for i, n in enumerate(kv_len):
        lo = 0 if window is None else max(0, n - window)
        qi = q[i, :, 0].double().view(kvh, h // kvh, d)
        p = torch.softmax(qi @ kd[i, :, lo:n].transpose(1, 2) * scale, dim=-1)
        out[i, :, 0] = (p @ vd[i, :, lo:n]).view(h, d)
    return out


@pytest.mark.parametrize("window", [None, 1, 200, 513])
@pytest.mark.parametrize("group", [1, 4, 7])
@pytest.mark.parametrize("hd", [64, 128])
def test_decode(hd, group, window):
    from libai_amd.ops.attention import flash_decode_attn_fp8

    q, k8, v8, ks, vs, kd, vd = _case(hd, group)
    scale = hd ** -0.5
    kv_len = torch.tensor(KV_LEN, dtype=torch.int32, device=DEV)
    out = flash_decode_attn_fp8(q, k8, v8, ks, vs, scale, kv_len=kv_len,
                                window=window)
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    ref = _reference(q, kd, vd, KV_LEN, window, scale)
    err = (out.double() - ref).abs().amax(dim=(1, 2, 3))
    print(f"hd{hd} g{group} w{window}: max-abs err per batch {err.tolist()}")
    assert float(err.max()) < FWD_TOL
    if window == 1:  # the window is applied: the long row is not the full one
        full = _reference(q, kd, vd, KV_LEN, None, scale)
        assert float((out[3].double() - full[3]).abs().max()) > FWD_TOL


@pytest.mark.parametrize("hd", [64, 128])
def test_decode_capacity_independent(hd):
    from libai_amd.ops.attention import flash_decode_attn_fp8

    q, k8, v8, ks, vs, _, _ = _case(hd, 4, cap=512, b=2)
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


# ---- decoders ---------------------------------------------------------------
def _tiny_llama():
    from libai_amd.models.llama import LlamaForCausalLM

    torch.manual_seed(1)
    m = LlamaForCausalLM(
        hidden_layers=2, vocab_size=1024, hidden_size=512,
        intermediate_size=512, num_attention_heads=8,
        num_key_value_heads=2, max_position_embeddings=128,
    )
    return m.to(DEV, torch.bfloat16).eval()


@torch.no_grad()
def _eager_static(dec, prompt, n_new):
    """The decoder's own static step, run without a graph from its prefill.
    -> (tokens [b, n_new], logits of the first decode step)."""
    L = prompt.shape[1]
    out = dec.model(input_ids=prompt, use_cache=True)
    dec._fill_caches(out["past_key_values"], L)
    first = dec._select(out["prediction_scores"][:, -1, :])
    dec.out_tokens = torch.zeros(prompt.shape[0], n_new, dtype=torch.int64,
                                 device=DEV)
    dec.out_tokens[:, 0:1] = first
    dec._reset_to(L, first)
    logits0 = dec._logits().float()
    dec._reset_to(L, first)
    for _ in range(n_new - 1):
        dec._step()
    return dec.out_tokens.clone(), logits0


def test_captured_llama_fp8():
    from libai_amd.inference.captured_decode import CapturedLlamaDecoder

    model = _tiny_llama()
    prompt = torch.randint(0, 1024, (2, 12), device=DEV)
    dec = CapturedLlamaDecoder(model, max_batch=2, max_seq_len=64,
                               kv_cache_dtype="fp8")
    k8, v8, k_scale, _, _ = dec.caches[0]
    assert k8.element_size() == 1 and v8.shape == (2, 2, 64, 64)
    assert k_scale.shape == (2, 2, 64) and k_scale.dtype == torch.float32
    got = dec.generate(prompt, 16)
    ref, logits8 = _eager_static(
        CapturedLlamaDecoder(model, 2, 64, kv_cache_dtype="fp8"), prompt, 16)
    assert torch.equal(got, ref), f"mismatch:\n{got}\nvs\n{ref}"
    _, logits16 = _eager_static(CapturedLlamaDecoder(model, 2, 64), prompt, 2)
    print("first decode step, fp8 vs bf16 cache: logits max-abs diff "
          f"{float((logits8 - logits16).abs().max()):.4f}")


def test_continuous_llama_fp8():
    from libai_amd.inference.captured_decode import (
        CapturedLlamaDecoder,
        ContinuousLlamaDecoder,
    )

    model = _tiny_llama()
    p0 = torch.randint(0, 1024, (1, 25), device=DEV)
    p1 = torch.randint(0, 1024, (1, 11), device=DEV)
    dec = ContinuousLlamaDecoder(model, max_batch=3, max_seq_len=64,
                                 kv_cache_dtype="fp8")
    dec.add_request(0, p0[0])
    dec.step(6)
    dec.add_request(2, p1[0])  # admitted mid-flight, non-contiguous slot
    dec.step(6)
    alone = CapturedLlamaDecoder(model, max_batch=1, max_seq_len=64,
                                 kv_cache_dtype="fp8")
    assert torch.equal(dec.tokens(0), alone.generate(p0, 13)[0])
    assert torch.equal(dec.tokens(2), alone.generate(p1, 7)[0])


def test_gpt_fp8_not_implemented():
    from libai_amd.inference.captured_decode import CapturedGPTDecoder
    from libai_amd.models.gpt_model import GPTForPreTraining

    m = GPTForPreTraining(hidden_layers=1, vocab_size=128, hidden_size=128,
                          ffn_hidden_size=256, num_attention_heads=2,
                          max_seq_length=32).to(DEV, torch.bfloat16)
    with pytest.raises(NotImplementedError):
        CapturedGPTDecoder(m, max_batch=1, max_seq_len=32, kv_cache_dtype="fp8")
