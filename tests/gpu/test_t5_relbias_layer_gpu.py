"""T5 relative-position bias through the layers: a bias that carries its
diagonal table takes the flash kernels (table gradient included) and agrees
with the materialized route, which the same bias without the attribute takes."""

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2    # max-abs (the project's bound for bf16 outputs)
GRAD_TOL = 5e-2   # relative to the other route's grad max-abs
# Model-level loss: both routes feed the same fp32 cross entropy from bf16
# logits; one bf16 rounding of an O(1) logit is 2^-8 ~ 4e-3 and the mean over
# tokens does not amplify it, so the project's max-abs output bound is used for
# the loss difference as well.
LOSS_TOL = FWD_TOL


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    yield


def _record(monkeypatch):
    """Wrap ops.attention.flash_attention_qkv, recording each call's table."""
    import libai_amd.ops.attention as A

    calls = []
    orig = A.flash_attention_qkv

    def wrapper(*a, **kw):
        calls.append(kw.get("rel_bias"))
        return orig(*a, **kw)

    monkeypatch.setattr(A, "flash_attention_qkv", wrapper)
    return calls


def _rel_err(got, want):
    return ((got.float() - want.float()).abs().max()
            / (want.float().abs().max() + 1e-6)).item()


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("mask_type", ["padding", "causal"])
def test_layer_rel_bias_fused_matches_materialized(monkeypatch, mask_type, padded):
    from libai_amd import layers
    from libai_amd.models.bert_model import extended_attn_mask

    torch.manual_seed(0)
    b, s, hidden, nh = 2, 200, 256, 4
    attn = layers.MultiheadAttention(hidden, nh, attn_mask_type=mask_type)
    attn = attn.to(torch.bfloat16).cuda().train()
    rel = layers.T5RelativePositionBias(nh, bidirectional=mask_type == "padding")
    rel = rel.to(torch.bfloat16).cuda()
    with torch.no_grad():  # the default init is small next to scale * q.k
        rel.weight.copy_(torch.randn_like(rel.weight) * 0.5)
    x = torch.randn(b, s, hidden, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(b, s, hidden, device="cuda", dtype=torch.bfloat16)
    mask, rows = None, torch.ones(b, s, device="cuda", dtype=torch.bool)
    if padded:
        lens = torch.tensor([s, 136], device="cuda")
        rows = torch.arange(s, device="cuda")[None, :] < lens[:, None]
        mask = extended_attn_mask(rows.to(torch.uint8))
        assert mask._kv_len is not None
        # loss-mask contract: padded query rows never reach the loss
        g = g * rows[:, :, None]

    calls = _record(monkeypatch)

    def run(fused):
        rel.weight.grad = None
        xi = x.clone().requires_grad_(True)
        bias = rel(s, s)
        if not fused:
            # the same values, attached to the graph, without the attribute
            bias = bias.clone()
            assert getattr(bias, "_rel_bias_table", None) is None
        n0 = len(calls)
        y = attn(xi, attention_mask=mask, position_bias=bias)
        if fused:
            assert len(calls) == n0 + 1 and calls[-1] is not None
            assert calls[-1].dtype == torch.float32
            assert tuple(calls[-1].shape) == (nh, 2 * s - 1)
        else:
            assert len(calls) == n0, "a bias without a table must not be fused"
        y.backward(g)
        return y.detach(), xi.grad, rel.weight.grad.clone()

    y_f, dx_f, dw_f = run(True)
    y_m, dx_m, dw_m = run(False)
    tag = f"layer {mask_type} padded{int(padded)}"
    err = ((y_f.float() - y_m.float()) * rows[:, :, None]).abs().max().item()
    print(f"[relbias-layer] {tag} out max err {err:.3e}")
    assert err < FWD_TOL, f"{tag} out max err {err}"
    for name, got, want in (("dx", dx_f, dx_m), ("dweight", dw_f, dw_m)):
        e = _rel_err(got, want)
        print(f"[relbias-layer] {tag} {name} rel err {e:.3e}")
        assert e < GRAD_TOL, f"{tag} {name} rel err {e}"
    assert dw_f.float().abs().max().item() > 0
    # the bias must matter at this shape, or the comparison shows nothing
    with torch.no_grad():
        y_none = attn(x, attention_mask=mask)
    assert ((y_f.float() - y_none.float()) * rows[:, :, None]).abs().max().item() \
        > FWD_TOL


@pytest.mark.parametrize("checkpoint", [False, True])
def test_t5_model_rel_bias_trains_through_flash(monkeypatch, checkpoint):
    import libai_amd.ops.attention as A
    from libai_amd.models import T5ForPreTraining

    torch.manual_seed(0)
    layers_n, b, s, vocab = 2, 2, 64, 512
    m = T5ForPreTraining(
        vocab_size=vocab, hidden_size=128, hidden_layers=layers_n,
        num_attention_heads=2, intermediate_size=256, max_position_embeddings=s,
        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
        embedding_dropout_prob=0.0, relative_attention=True,
    ).to(torch.bfloat16).cuda().train()
    m.set_activation_checkpoint(checkpoint)
    t5 = m.t5_model
    with torch.no_grad():
        for rb in (t5.enc_rel_bias, t5.dec_rel_bias):
            rb.weight.copy_(torch.randn_like(rb.weight) * 0.5)
    batch = dict(
        encoder_input_ids=torch.randint(0, vocab, (b, s), device="cuda"),
        decoder_input_ids=torch.randint(0, vocab, (b, s), device="cuda"),
        encoder_attn_mask=torch.ones(b, s, dtype=torch.uint8, device="cuda"),
        lm_labels=torch.randint(0, vocab, (b, s), device="cuda"),
        loss_mask=torch.ones(b, s, dtype=torch.long, device="cuda"),
    )
    calls = _record(monkeypatch)

    def run():
        m.zero_grad(set_to_none=True)
        n0 = len(calls)
        loss = m(**batch)["masked_lm_loss"]
        n_fwd = len(calls) - n0
        loss.backward()
        return (loss.item(), t5.enc_rel_bias.weight.grad.clone(),
                t5.dec_rel_bias.weight.grad.clone(), n_fwd, calls[n0:])

    loss_f, enc_f, dec_f, n_fwd, seen = run()
    # every self-attention layer, encoder and decoder, took the fused route
    # (checkpointing replays each forward once more during backward)
    assert n_fwd == 2 * layers_n
    assert len(seen) == (2 if checkpoint else 1) * 2 * layers_n
    assert all(t is not None for t in seen)

    # materialized route: the layers see no table
    monkeypatch.setattr(A, "bias_rel_table", lambda bias: None)
    loss_m, enc_m, dec_m, _, seen_m = run()
    assert seen_m == []

    tag = f"t5 ckpt{int(checkpoint)}"
    print(f"[relbias-layer] {tag} loss fused {loss_f:.5f} materialized {loss_m:.5f}")
    assert abs(loss_f - loss_m) < LOSS_TOL
    for name, got, want in (("enc dweight", enc_f, enc_m), ("dec dweight", dec_f, dec_m)):
        assert torch.isfinite(got.float()).all()
        assert got.float().abs().max().item() > 0
        e = _rel_err(got, want)
        print(f"[relbias-layer] {tag} {name} rel err {e:.3e}")
        assert e < GRAD_TOL, f"{tag} {name} rel err {e}"
