#!/usr/bin/env python3
"""Packed-document attention A/B: `flash_attention` fwd+bwd with document
bounds against the plain causal call, and a Llama decoder layer on a packed
row through the flash path against the unfused mask path.

Kernel level (b4 h16 D64 S1024 causal by default):
  plain    no doc_bounds: the DOCS=false instantiation every caller ran before
  one      doc_bounds, one document per row: the price of the variant
  8x128    doc_bounds, eight documents of 128 per row
  random   doc_bounds, seeded random lengths of mean 128
Next to each time the tool prints the share of the plain call's forward
staging rounds the layout walks (computed from the shapes, not measured).

Layer level: LlamaDecoderLayer fwd+bwd on the random layout, flash vs unfused,
time and peak allocated memory.

The variants are timed alternately, several rounds each; the median and
min..max of the per-round means are shown.  `--trace-pass N [--only LAYOUT]`
runs the kernel variants N times each and nothing else: the workload for a
kernel trace.

Usage (GPU box): python tools/packed_docs_bench.py [--steps 50] [--rounds 5]
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


def random_lengths(s, mean, seed):
    """Seeded document lengths, uniform on [1, 2 * mean - 1], cut at s."""
    g = torch.Generator().manual_seed(seed)
    lengths, left = [], s
    while left > 0:
        n = min(int(torch.randint(1, 2 * mean, (1,), generator=g)), left)
        lengths.append(n)
        left -= n
    return lengths


def layouts(b, s, mean, seed):
    return {
        "one": [[s]] * b,
        f"{s // mean}x{mean}": [[mean] * (s // mean)] * b,
        "random": [random_lengths(s, mean, seed + r) for r in range(b)],
    }


def bounds(rows, s):
    from libai_amd.data.packing import doc_bounds_from_lengths

    per_row = [doc_bounds_from_lengths(r, s) for r in rows]
    return (torch.stack([p[0] for p in per_row]).cuda().contiguous(),
            torch.stack([p[1] for p in per_row]).cuda().contiguous())


def fwd_rounds_visited(s, rows):
    """Staging rounds of FWD_ROUND keys the forward's workgroups walk; rows =
    None is the plain causal call."""
    total = 0
    for row in rows or [[s]]:
        starts, a = [], 0
        for n in row:
            starts += [a] * n
            a += n
        for q_block in range(0, s, QBLK):
            hi = -(-min(s, q_block + QBLK) // FWD_ROUND)
            total += hi - starts[q_block] // FWD_ROUND
    return total / len(rows or [0])


def bench_kernels(args):
    from libai_amd.ops.attention import flash_attention

    b, s, h, d = args.batch, args.seq, args.heads, args.head_dim
    torch.manual_seed(0)
    mk = lambda: torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16,
                             requires_grad=True)
    q, k, v = mk(), mk(), mk()
    g = torch.randn(b, s, h, d, device="cuda", dtype=torch.bfloat16)
    scale = d ** -0.5
    lay = layouts(b, s, args.mean_doc, args.seed)
    doc_bounds = {"plain": None}
    doc_bounds.update({n: bounds(rows, s) for n, rows in lay.items()})

    def fwd(db):
        def fn():
            with torch.no_grad():
                flash_attention(q, k, v, scale, causal=True, doc_bounds=db)
        return fn

    def fwd_bwd(db):
        def fn():
            q.grad = k.grad = v.grad = None
            flash_attention(q, k, v, scale, causal=True, doc_bounds=db).backward(g)
        return fn

    if args.trace_pass:
        for n, db in doc_bounds.items():
            if args.only and n != args.only:
                continue
            for _ in range(args.trace_pass):
                fwd_bwd(db)()
            torch.cuda.synchronize()
        return

    res_f = _ab({n: fwd(db) for n, db in doc_bounds.items()}, args.steps, args.rounds)
    res_fb = _ab({n: fwd_bwd(db) for n, db in doc_bounds.items()}, args.steps,
                 args.rounds)
    base = fwd_rounds_visited(s, None)
    print(f"## flash_attention, b{b} h{h} D{d} S{s} causal, bf16\n")
    print("| layout | documents per row | fwd ms (median) | fwd min..max | "
          "fwd+bwd ms (median) | fwd+bwd min..max | fwd+bwd vs plain | "
          "fwd rounds walked vs plain |")
    print("|---|---|---|---|---|---|---|---|")
    for n in doc_bounds:
        f, fb = res_f[n], res_fb[n]
        rows = lay.get(n)
        ndoc = "-" if rows is None else "/".join(str(len(r)) for r in rows)
        print(f"| {n} | {ndoc} | {f[0]:.4f} | {f[1]:.4f}..{f[2]:.4f} | {fb[0]:.4f} | "
              f"{fb[1]:.4f}..{fb[2]:.4f} | {fb[0] / res_fb['plain'][0]:.3f} | "
              f"{fwd_rounds_visited(s, rows) / base:.3f} |")
    print()


def bench_layer(args):
    import libai_amd.models.llama as L
    from libai_amd.models.utils.weight_init import init_method_normal

    b, s, h, d = args.batch, args.seq, args.heads, args.head_dim
    hidden = h * d
    torch.manual_seed(0)
    init = init_method_normal(0.02)
    layer = L.LlamaDecoderLayer(hidden, 4 * hidden * 2 // 3 // 64 * 64, h, s, 1e-5,
                                init, init).to("cuda", torch.bfloat16).train()
    x = torch.randn(b, s, hidden, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    g = torch.randn_like(x)
    ds, de = bounds(layouts(b, s, args.mean_doc, args.seed)["random"], s)
    available = L.flash_attention_available

    def route(flash):
        def fn():
            L.flash_attention_available = available if flash else (lambda *a, **k: False)
            try:
                x.grad = None
                layer.zero_grad(set_to_none=True)
                layer(x, doc_start=ds, doc_end=de).backward(g)
            finally:
                L.flash_attention_available = available
        return fn

    routes = {"flash (DOCS kernels)": route(True), "unfused mask path": route(False)}
    res = _ab(routes, args.layer_steps, args.rounds)
    peak = {}
    for n, fn in routes.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    print(f"## LlamaDecoderLayer fwd+bwd, b{b} S{s} hidden {hidden} h{h} D{d}, "
          f"random layout (mean {args.mean_doc}), bf16\n")
    print("| attention path | ms (median) | min..max | peak allocated above the "
          "resident tensors, MiB |")
    print("|---|---|---|---|")
    for n in routes:
        m = res[n]
        print(f"| {n} | {m[0]:.3f} | {m[1]:.3f}..{m[2]:.3f} | {peak[n]:.1f} |")
    print()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--heads", type=int, default=16)
    p.add_argument("--head-dim", type=int, default=64)
    p.add_argument("--mean-doc", type=int, default=128)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--layer-steps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--trace-pass", type=int, default=0, metavar="N",
                   help="run each kernel variant N times and exit")
    p.add_argument("--only", default=None,
                   help="with --trace-pass: run this variant alone (the layouts "
                        "share their kernels' names)")
    args = p.parse_args()
    assert torch.cuda.is_available(), "packed_docs_bench needs a GPU"

    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    bench_kernels(args)
    if not args.trace_pass:
        bench_layer(args)


if __name__ == "__main__":
    main()
