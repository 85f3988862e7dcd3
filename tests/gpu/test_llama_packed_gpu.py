"""Llama on a packed row: attention and RoPE stay inside each document, through
the flash (DOCS) kernels."""

import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.1  # model logits, as in tests/gpu/test_flash_window_gpu.py
S, DOCS = 128, [40, 88]


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _tiny_llama(kv_heads=None):
    from libai_amd.models.llama import LlamaForCausalLM

    torch.manual_seed(1)
    m = LlamaForCausalLM(
        hidden_layers=2, vocab_size=1024, hidden_size=256, intermediate_size=512,
        num_attention_heads=4, num_key_value_heads=kv_heads,
        max_position_embeddings=256,
    )
    return m.to("cuda", torch.bfloat16)


def _batch():
    from libai_amd.data.packing import doc_bounds_from_lengths

    torch.manual_seed(2)
    ids = torch.randint(0, 1024, (2, S), device="cuda")
    ds, de, _ = doc_bounds_from_lengths(DOCS, S)
    ds = ds[None].expand(2, S).contiguous().cuda()
    de = de[None].expand(2, S).contiguous().cuda()
    return ids, ds, de


def _spy_flash_fwd(monkeypatch):
    """Wrap ext().flash_fwd, recording whether each call carried doc bounds."""
    from libai_amd.ops._ext import ext

    calls = []
    orig = ext().flash_fwd

    def wrapper(*a, **kw):
        ds = kw.get("doc_start", a[11] if len(a) > 11 else None)
        de = kw.get("doc_end", a[12] if len(a) > 12 else None)
        calls.append(ds is not None and de is not None)
        return orig(*a, **kw)

    monkeypatch.setattr(ext(), "flash_fwd", wrapper)
    return calls


@pytest.mark.parametrize("kv_heads", [None, 1])
def test_packed_logits_match_each_document_alone(monkeypatch, kv_heads):
    model = _tiny_llama(kv_heads).eval()
    ids, ds, de = _batch()
    calls = _spy_flash_fwd(monkeypatch)
    with torch.no_grad():
        packed = model(input_ids=ids, doc_start=ds, doc_end=de)["prediction_scores"]
        assert calls == [True, True], calls  # one flash call per layer, with bounds
        plain = model(input_ids=ids)["prediction_scores"]
        a = 0
        for n in DOCS:
            alone = model(input_ids=ids[:, a:a + n])["prediction_scores"]
            err = (packed[:, a:a + n].float() - alone.float()).abs().max().item()
            print(f"kv_heads {kv_heads} doc@{a}+{n} logits max diff {err:.3e}")
            assert err < LOGIT_TOL, err
            a += n
    assert calls == [True, True] + [False] * 6, calls
    # the second document must differ from the unpacked run, or the comparison
    # above shows nothing
    assert (packed[:, DOCS[0]:].float() - plain[:, DOCS[0]:].float()).abs().max() \
        > LOGIT_TOL


@pytest.mark.parametrize("kv_heads", [None, 1])
def test_packed_training_step_is_finite(monkeypatch, kv_heads):
    model = _tiny_llama(kv_heads).train()
    ids, ds, de = _batch()
    labels = torch.roll(ids, -1, dims=1)
    labels[:, de[0].long().unique() - 1] = -100  # each document's last token
    calls = _spy_flash_fwd(monkeypatch)
    loss = sum(model(input_ids=ids, labels=labels, doc_start=ds, doc_end=de).values())
    loss.backward()
    assert calls == [True, True], calls
    assert torch.isfinite(loss).item()
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        assert torch.isfinite(p.grad.float()).all(), name


def test_packed_rejects_cache_and_window():
    from libai_amd.models.llama import LlamaForCausalLM

    model = _tiny_llama().eval()
    ids, ds, de = _batch()
    with torch.no_grad():
        with pytest.raises(ValueError):
            model(input_ids=ids, doc_start=ds, doc_end=de, use_cache=True)
        with pytest.raises(ValueError):
            model(input_ids=ids, doc_start=ds)
        past = model(input_ids=ids[:, :8], use_cache=True)["past_key_values"]
        with pytest.raises(ValueError):
            model(input_ids=ids[:, 8:9], past_key_values=past, doc_start=ds[:, 8:9],
                  doc_end=de[:, 8:9])
    torch.manual_seed(1)
    windowed = LlamaForCausalLM(
        hidden_layers=1, vocab_size=1024, hidden_size=256, intermediate_size=512,
        num_attention_heads=4, max_position_embeddings=256, sliding_window=16,
    ).to("cuda", torch.bfloat16).eval()
    with torch.no_grad(), pytest.raises(ValueError):
        windowed(input_ids=ids, doc_start=ds, doc_end=de)
