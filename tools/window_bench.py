#!/usr/bin/env python3
"""Sliding-window attention A/B at the kernel level: `flash_attention`
fwd+bwd and `flash_decode_attn` with and without a window.

window=None runs the windowless instantiation (the kernel every caller had
before the window existed) and is the baseline.  For each windowed shape the
fraction of tiles the kernel visits is printed next to the time ratio, so a
reader can see how close the time comes to the work.

Training: b1 h32 kvh8 D128 S8192 causal (the configs/mistral_7b_pretrain.py
attention), window in {None, 4096, 1024, 256}.
Decode: b8 h32 kvh8 D128, kv_len in {2048, 8192} (cache capacity = kv_len),
window in {None, 4096, 1024}.

The variants are timed alternately, several rounds each; the median of the
per-round means is shown.

Usage (GPU box): python tools/window_bench.py [--steps 20] [--rounds 5]
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

QBLK = 128        # query rows per workgroup (fwd, bwd_q); kv rows in bwd_kv
FWD_ROUND = 128   # keys staged per forward round
CHUNK = 64        # keys per decode chunk


def _timed(fn, steps):
    """ms per call: host clock around device-synchronized work."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _ab(routes, steps, rounds, warmup=3):
    """routes: {name: fn}.  Alternates the routes round by round."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    ms = {n: [] for n in routes}
    for _ in range(rounds):
        for n, fn in routes.items():
            ms[n].append(_timed(fn, steps))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in ms.items()}


def fwd_rounds_visited(s, window):
    """Staging rounds of FWD_ROUND keys the forward's workgroups walk (the
    backward kernels cut their loops at the same band edges)."""
    total = 0
    for q_block in range(0, s, QBLK):
        hi = -(-min(s, q_block + QBLK) // FWD_ROUND)
        lo = 0 if not window else max(0, q_block - window + 1) // FWD_ROUND
        total += hi - lo
    return total


def decode_chunks_visited(kv_len, window):
    lo = 0 if not window else max(0, kv_len - window)
    return -(-kv_len // CHUNK) - lo // CHUNK


def _wname(w):
    return "None" if w is None else str(w)


def bench_train(args):
    from libai_amd.ops.attention import flash_attention

    b, s, h, hkv, d = args.batch, args.seq, args.heads, args.kv_heads, args.head_dim
    torch.manual_seed(0)
    mk = lambda n: torch.randn(b, s, n, d, device="cuda", dtype=torch.bfloat16,
                               requires_grad=True)
    q, k, v = mk(h), mk(hkv), mk(hkv)
    g = torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16)
    scale = d ** -0.5

    def fwd(w):
        def fn():
            with torch.no_grad():
                flash_attention(q, k, v, scale, causal=True, window=w)
        return fn

    def fwd_bwd(w):
        def fn():
            q.grad = k.grad = v.grad = None
            flash_attention(q, k, v, scale, causal=True, window=w).backward(g)
        return fn

    windows = [None] + [w for w in args.windows if w < s]
    res_f = _ab({_wname(w): fwd(w) for w in windows}, args.steps, args.rounds)
    res_fb = _ab({_wname(w): fwd_bwd(w) for w in windows}, args.steps, args.rounds)
    base_tiles = fwd_rounds_visited(s, None)
    print(f"## flash_attention, b{b} h{h} kvh{hkv} D{d} S{s} causal, bf16\n")
    print("| window | fwd ms (median) | fwd min..max | fwd+bwd ms (median) | "
          "fwd+bwd min..max | fwd+bwd vs None | tiles visited vs None |")
    print("|---|---|---|---|---|---|---|")
    for w in windows:
        n = _wname(w)
        f, fb = res_f[n], res_fb[n]
        print(f"| {n} | {f[0]:.3f} | {f[1]:.3f}..{f[2]:.3f} | {fb[0]:.3f} | "
              f"{fb[1]:.3f}..{fb[2]:.3f} | {fb[0] / res_fb['None'][0]:.3f} | "
              f"{fwd_rounds_visited(s, w) / base_tiles:.3f} |")
    print()


def bench_decode(args):
    from libai_amd.ops.attention import flash_decode_attn

    b, h, hkv, d = args.decode_batch, args.heads, args.kv_heads, args.head_dim
    scale = d ** -0.5
    print(f"## flash_decode_attn, b{b} h{h} kvh{hkv} D{d}, cache capacity = "
          f"kv_len, bf16\n")
    print("| kv_len | window | us (median) | us min..max | vs None | "
          "chunks visited vs None |")
    print("|---|---|---|---|---|---|")
    for kv_len in args.kv_lens:
        torch.manual_seed(0)
        q = torch.randn(b, h, 1, d, device="cuda", dtype=torch.bfloat16)
        k = torch.randn(b, hkv, kv_len, d, device="cuda", dtype=torch.bfloat16)
        v = torch.randn_like(k)
        lens = torch.full((b,), kv_len, device="cuda", dtype=torch.int32)

        def dec(w):
            def fn():
                with torch.no_grad():
                    flash_decode_attn(q, k, v, scale, kv_len=lens, window=w)
            return fn

        windows = [None] + [w for w in args.decode_windows if w < kv_len]
        res = _ab({_wname(w): dec(w) for w in windows}, args.decode_steps,
                  args.rounds)
        base = decode_chunks_visited(kv_len, None)
        for w in windows:
            m = res[_wname(w)]
            print(f"| {kv_len} | {_wname(w)} | {m[0] * 1e3:.1f} | "
                  f"{m[1] * 1e3:.1f}..{m[2] * 1e3:.1f} | "
                  f"{m[0] / res['None'][0]:.3f} | "
                  f"{decode_chunks_visited(kv_len, w) / base:.3f} |")
    print()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--seq", type=int, default=8192)
    p.add_argument("--heads", type=int, default=32)
    p.add_argument("--kv-heads", type=int, default=8)
    p.add_argument("--head-dim", type=int, default=128)
    p.add_argument("--windows", type=int, nargs="+", default=[4096, 1024, 256])
    p.add_argument("--decode-batch", type=int, default=8)
    p.add_argument("--kv-lens", type=int, nargs="+", default=[2048, 8192])
    p.add_argument("--decode-windows", type=int, nargs="+", default=[4096, 1024])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--decode-steps", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "window_bench needs a GPU"

    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    bench_train(args)
    bench_decode(args)


if __name__ == "__main__":
    main()
