#!/usr/bin/env python3
"""BLOOM attention A/B: ALiBi fused into the flash / decode kernels (the bias
carries its fp32 slopes) vs the materialized-scores route a plain bias tensor
takes (bmm -> +bias -> unfused softmax -> bmm).

One BLOOM TransformerLayer at the configs/bloom_pretrain.py shape (b4, s1024,
h1024, 16 heads, bf16, dropout 0.1): training fwd+bwd, and single-token decode
against a 1024-key cache.  Reports ms and peak allocated memory per route.
The two routes are timed alternately, several rounds each; the median is shown.

Usage (GPU box): python tools/alibi_bench.py [--steps 20] [--rounds 5]
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
    print(f"\nfused vs materialized: {b / f:.2f}x "
          f"({100 * (f - b) / b:+.1f}% time), "
          f"peak {res[base][3] / 2**20:.1f} -> {res[new][3] / 2**20:.1f} MB\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--hidden", type=int, default=1024)
    p.add_argument("--heads", type=int, default=16)
    p.add_argument("--dropout", type=float, default=0.1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "alibi_bench needs a GPU"

    import bench as bench_mod

    bench_mod._enable_tuned_gemms()
    import libai_amd.ops.attention as A
    from libai_amd.layers import AttnMaskType, TransformerLayer
    from libai_amd.layers.position_bias import build_alibi_bias
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    torch.manual_seed(0)
    layer = TransformerLayer(
        args.hidden, 4 * args.hidden, args.heads,
        attention_dropout_prob=args.dropout, output_dropout_prob=args.dropout,
        attn_mask_type=AttnMaskType.causal,
    ).to(torch.bfloat16).cuda()

    b, s = args.batch, args.seq
    fused_bias = build_alibi_bias(args.heads, s, device="cuda", dtype=torch.bfloat16)
    plain_bias = fused_bias.clone()  # same values, no slopes attached
    assert A.bias_alibi_slopes(fused_bias) is not None
    assert A.bias_alibi_slopes(plain_bias) is None

    # which route ran is checked, not assumed
    calls = {"flash": 0, "decode": 0}
    orig_qkv, orig_dec = A.flash_attention_qkv, A.flash_decode_attn

    def count_qkv(*a, **k):
        calls["flash"] += 1
        return orig_qkv(*a, **k)

    def count_dec(*a, **k):
        calls["decode"] += 1
        return orig_dec(*a, **k)

    A.flash_attention_qkv, A.flash_decode_attn = count_qkv, count_dec

    # ---- training fwd+bwd -------------------------------------------------
    layer.train()
    x = torch.randn(b, s, args.hidden, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    g = torch.randn(b, s, args.hidden, device="cuda", dtype=torch.bfloat16)

    def train_step(bias):
        def fn():
            layer.zero_grad(set_to_none=True)
            x.grad = None
            layer(x, position_bias=bias).backward(g)
        return fn

    n0 = calls["flash"]
    train_step(plain_bias)()
    assert calls["flash"] == n0, "plain bias must take the materialized route"
    train_step(fused_bias)()
    assert calls["flash"] == n0 + 1, "ALiBi bias must take the flash route"
    res = _ab({"materialized bias": train_step(plain_bias),
               "fused ALiBi (flash)": train_step(fused_bias)},
              args.steps, args.rounds)
    print(f"# BLOOM layer, b{b} s{s} h{args.hidden} nh{args.heads} bf16, "
          f"dropout {args.dropout}\n")
    _report("train fwd+bwd (one TransformerLayer)", res, "materialized bias",
            "fused ALiBi (flash)")

    # ---- single-token decode at kv = seq ------------------------------------
    layer.eval()
    layer.zero_grad(set_to_none=True)
    hd = args.hidden // args.heads
    pk = torch.randn(b, args.heads, s - 1, hd, device="cuda", dtype=torch.bfloat16)
    pv = torch.randn_like(pk)
    tok = torch.randn(b, 1, args.hidden, device="cuda", dtype=torch.bfloat16)

    def decode_step(bias):
        def fn():
            with torch.no_grad():
                layer(tok, position_bias=bias, past_key_value=(pk, pv),
                      use_cache=True)
        return fn

    n0 = calls["decode"]
    decode_step(plain_bias)()
    assert calls["decode"] == n0, "plain bias must take the unfused decode"
    decode_step(fused_bias)()
    assert calls["decode"] == n0 + 1, "ALiBi bias must take the fused decode"
    res = _ab({"materialized bias": decode_step(plain_bias),
               "fused ALiBi (flash_decode)": decode_step(fused_bias)},
              max(args.steps, 50), args.rounds)
    _report(f"single-token decode, kv {s} (one TransformerLayer, incl. the "
            f"cache concat)", res, "materialized bias",
            "fused ALiBi (flash_decode)")


if __name__ == "__main__":
    main()
