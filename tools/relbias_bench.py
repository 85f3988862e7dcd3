#!/usr/bin/env python3
"""MT5 attention A/B: the T5 relative-position bias fused into the flash
kernels (the bias carries its fp32 diagonal table; the backward returns the
table gradient) vs the materialized-scores route the same bias takes without
the table (bmm -> +bias -> unfused softmax -> bmm).

At the configs/mt5_pretrain.py shape (b16, encoder s512, h768, 12 heads of 64,
gated-gelu MLP, bf16, dropout 0.1), training fwd+bwd of
  * one encoder TransformerLayer (bidirectional bias, padding mask type),
  * one decoder self-attention block (causal, unidirectional bias),
  * the bare flash_attention_qkv call with and without a table.
The model builds the bias once per stack and every layer of the stack adds
its bias (or table) gradient to it, so the layer rows take the bias as a leaf
that requires grad -- the [1, nh, s, s] tensor on the materialized route, the
[nh, 2s-1] table on the fused one -- and a row of its own times the bias
module (forward, and backward from a gradient of the matching shape), the
once-per-stack cost.  Routes are timed alternately, several rounds each;
median, min..max and peak allocated memory are shown.  Which route ran is
asserted, not assumed.

The config's decoder length (114) is not a multiple of 8, which the flash
kernels require, so that self-attention keeps the materialized route with or
without a table; the decoder row therefore runs at --dec-seq (default 120).

Usage (GPU box): python tools/relbias_bench.py [--steps 10] [--rounds 5]
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def _timed(fn, steps):
    """ms per call (host clock around device-synchronized work) and the peak
    allocated bytes above the level held before the call."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return ms, torch.cuda.max_memory_allocated() - base


def _ab(routes, steps, rounds, warmup=3):
    """routes: {name: fn}.  Alternates the routes round by round."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    ms = {n: [] for n in routes}
    peak = {n: 0 for n in routes}
    for _ in range(rounds):
        for n, fn in routes.items():
            t, p = _timed(fn, steps)
            ms[n].append(t)
            peak[n] = max(peak[n], p)
    return {n: (statistics.median(ms[n]), min(ms[n]), max(ms[n]), peak[n])
            for n in routes}


def _report(title, res, base, new):
    print(f"## {title}")
    print("| route | ms (median) | ms (min..max) | peak MB |")
    print("|---|---|---|---|")
    for n, (med, lo, hi, pk) in res.items():
        print(f"| {n} | {med:.3f} | {lo:.3f}..{hi:.3f} | {pk / 2**20:.1f} |")
    b, f = res[base][0], res[new][0]
    print(f"\n{new} vs {base}: {b / f:.2f}x "
          f"({100 * (f - b) / b:+.1f}% time), "
          f"peak {res[base][3] / 2**20:.1f} -> {res[new][3] / 2**20:.1f} MB\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--seq", type=int, default=512)
    p.add_argument("--dec-seq", type=int, default=120)
    p.add_argument("--hidden", type=int, default=768)
    p.add_argument("--heads", type=int, default=12)
    p.add_argument("--dropout", type=float, default=0.1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "relbias_bench needs a GPU"

    import bench as bench_mod

    bench_mod._enable_tuned_gemms()
    import libai_amd.ops.attention as A
    from libai_amd.layers import (AttnMaskType, MultiheadAttention,
                                  T5RelativePositionBias, TransformerLayer)
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    torch.manual_seed(0)
    b, hid, nh = args.batch, args.hidden, args.heads
    hd = hid // nh

    # which route ran is checked, not assumed
    calls = {"flash": 0, "table": 0}
    orig_qkv = A.flash_attention_qkv

    def count_qkv(*a, **k):
        calls["flash"] += 1
        calls["table"] += k.get("rel_bias") is not None
        return orig_qkv(*a, **k)

    A.flash_attention_qkv = count_qkv

    def ab_module(title, module, rel, s):
        module.train()
        x = torch.randn(b, s, hid, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        g = torch.randn(b, s, hid, device="cuda", dtype=torch.bfloat16)

        with torch.no_grad():
            built = rel(s, s)
        table = built._rel_bias_table.clone().requires_grad_(True)
        fused_bias = built.clone()
        fused_bias._rel_bias_table = table
        plain_bias = built.clone().requires_grad_(True)  # no table attached

        def step(fused):
            bias, leaf = (fused_bias, table) if fused else (plain_bias, plain_bias)

            def fn():
                module.zero_grad(set_to_none=True)
                x.grad = leaf.grad = None
                module(x, position_bias=bias).backward(g)
                assert leaf.grad is not None and leaf.grad.shape == leaf.shape
            return fn

        n0 = dict(calls)
        step(False)()
        assert calls == n0, "a bias without a table must take the materialized route"
        step(True)()
        assert calls["flash"] == n0["flash"] + 1 and calls["table"] == n0["table"] + 1, \
            "a bias with a table must take the flash route"
        print(f"route check: {title}: table -> flash kernels, no table -> "
              f"materialized scores")
        res = _ab({"materialized bias": step(False),
                   "fused table (flash)": step(True)}, args.steps, args.rounds)
        _report(title, res, "materialized bias", "fused table (flash)")

    def ab_bias_module(title, rel, s):
        gb = torch.randn(1, nh, s, s, device="cuda", dtype=torch.bfloat16)
        gt = torch.randn(nh, 2 * s - 1, device="cuda")

        def step(fused):
            def fn():
                rel.zero_grad(set_to_none=True)
                bias = rel(s, s)
                if fused:
                    bias._rel_bias_table.backward(gt)
                else:
                    bias.backward(gb)
                assert rel.weight.grad is not None
            return fn

        res = _ab({"bias gradient [1, nh, s, s]": step(False),
                   "table gradient [nh, 2s-1]": step(True)}, args.steps, args.rounds)
        _report(title, res, "bias gradient [1, nh, s, s]", "table gradient [nh, 2s-1]")

    print(f"# MT5 relative-position bias, b{b} h{hid} nh{nh} d{hd} bf16, "
          f"dropout {args.dropout}\n")

    # ---- encoder layer ------------------------------------------------------
    enc = TransformerLayer(
        hid, 4 * hid, nh, attention_dropout_prob=args.dropout,
        output_dropout_prob=args.dropout, attn_mask_type=AttnMaskType.padding,
        mlp_type="gated", activation="gelu",
    ).to(torch.bfloat16).cuda()
    enc_rel = T5RelativePositionBias(nh, bidirectional=True).to(torch.bfloat16).cuda()
    ab_module(f"encoder TransformerLayer, s{args.seq}, train fwd+bwd", enc, enc_rel,
              args.seq)
    del enc
    ab_bias_module(f"T5RelativePositionBias fwd+bwd, s{args.seq} (once per stack)",
                   enc_rel, args.seq)

    # ---- decoder self-attention ------------------------------------------------
    assert not A.flash_attention_available(hd, torch.bfloat16, torch.device("cuda"),
                                           114, 114, None), \
        "s114 is expected to stay off the flash kernels (Sk % 8)"
    print("note: the config's decoder length 114 is not a multiple of 8: its "
          "self-attention is materialized on both routes\n")
    dec = MultiheadAttention(
        hid, nh, attention_dropout_prob=args.dropout,
        output_dropout_prob=args.dropout, attn_mask_type=AttnMaskType.causal,
    ).to(torch.bfloat16).cuda()
    dec_rel = T5RelativePositionBias(nh, bidirectional=False).to(torch.bfloat16).cuda()
    ab_module(f"decoder self-attention, causal, s{args.dec_seq}, train fwd+bwd",
              dec, dec_rel, args.dec_seq)
    ab_module(f"decoder self-attention, causal, s{args.seq}, train fwd+bwd",
              dec, dec_rel, args.seq)
    del dec

    # ---- kernel level -----------------------------------------------------------
    s = args.seq
    for causal in (False, True):
        qkv = torch.randn(b, s, nh, 3, hd, device="cuda", dtype=torch.bfloat16,
                          requires_grad=True)
        table = (torch.randn(nh, 2 * s - 1, device="cuda") * 0.5).requires_grad_(True)
        g = torch.randn(b, s, nh, hd, device="cuda", dtype=torch.bfloat16)

        def kstep(t):
            def fn():
                qkv.grad = None
                if t is not None:
                    t.grad = None
                orig_qkv(qkv, hd ** -0.5, p_drop=args.dropout, causal=causal,
                         rel_bias=t).backward(g)
                assert t is None or t.grad is not None
            return fn

        res = _ab({"no bias": kstep(None), "table + dtable": kstep(table)},
                  args.steps, args.rounds)
        _report(f"flash_attention_qkv fwd+bwd, s{s}, causal={causal}", res,
                "no bias", "table + dtable")


if __name__ == "__main__":
    main()
