#!/usr/bin/env python3
"""FP8 KV cache against the bf16 cache (profiles/kv_fp8_decode.md).

Kernel level: flash_decode_attn_fp8 against flash_decode_attn at batch 32, the
two alternated inside one process, device events around runs of --iters calls,
--rounds rounds per version (median and min..max reported).  Achieved bytes/s
uses the bytes each format must read once: K and V data plus the fp32 scales.
End to end (--e2e): the captured Llama-1B-GQA step at b32 ctx1024 on both
caches, and the cache bytes a layer allocates.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # us per call


def _alternate(fns, iters, rounds):
    for fn in fns.values():  # warm every shape the timed window uses
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(_time(fn, iters))
    return times


def kernel_level(args):
    from libai_amd.ops.attention import flash_decode_attn, flash_decode_attn_fp8

    b = 32
    geoms = [("Llama-GQA", 32, 8, 128), ("Qwen2-like", 28, 4, 128),
             ("D64 G4", 32, 8, 64), ("MHA G1", 16, 16, 128)]
    print("| geometry | ctx | bf16 us (min..max) | fp8 us (min..max) | bf16/fp8 | "
          "bf16 TB/s | fp8 TB/s | max-abs diff |")
    print("|---|---|---|---|---|---|---|---|")
    for name, h, kvh, d in geoms:
        for ctx in (1024, 4096):
            torch.manual_seed(0)
            q = torch.randn(b, h, 1, d, device="cuda", dtype=torch.bfloat16)
            k = torch.randn(b, kvh, ctx, d, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(b, kvh, ctx, d, device="cuda", dtype=torch.bfloat16)
            kv_len = torch.full((b,), ctx, dtype=torch.int32, device="cuda")
            caches = []
            for x in (k, v):
                scale = x.float().abs().amax(-1) / 448.0
                c8 = (x.float() / scale[..., None]).clamp(-448, 448)
                caches += [c8.to(torch.float8_e4m3fn).view(torch.uint8), scale]
            k8, ks, v8, vs = caches
            sm = d ** -0.5
            fns = {
                "bf16": lambda: flash_decode_attn(q, k, v, sm, kv_len=kv_len),
                "fp8": lambda: flash_decode_attn_fp8(q, k8, v8, ks, vs, sm,
                                                     kv_len=kv_len),
            }
            diff = float((fns["bf16"]().float() - fns["fp8"]().float()).abs().max())
            t = _alternate(fns, args.iters, args.rounds)
            med = {n: statistics.median(x) for n, x in t.items()}
            rows = b * kvh * ctx
            need = {"bf16": rows * 2 * d * 2, "fp8": rows * (2 * d + 8)}
            cell = {n: f"{med[n]:.1f} ({min(t[n]):.1f}..{max(t[n]):.1f})" for n in t}
            print(f"| {name} H{h} KVH{kvh} D{d} | {ctx} | {cell['bf16']} | "
                  f"{cell['fp8']} | {med['bf16'] / med['fp8']:.2f}x | "
                  f"{need['bf16'] / med['bf16'] * 1e-6:.2f} | "
                  f"{need['fp8'] / med['fp8'] * 1e-6:.2f} | {diff:.4f} |", flush=True)


def end_to_end(args):
    from libai_amd.inference.captured_decode import CapturedLlamaDecoder
    from libai_amd.models import LlamaForCausalLM

    torch.manual_seed(0)
    model = LlamaForCausalLM(
        hidden_layers=16, vocab_size=32000, hidden_size=2048,
        intermediate_size=5504, num_attention_heads=16,
        num_key_value_heads=4, max_position_embeddings=4096,
    ).to(torch.bfloat16).cuda().eval()
    # every replay writes one column of the decoder's token buffer: generate
    # sizes it for `new` tokens, so a timed run replays fewer steps than that
    b, ctx, new, steps = 32, 1024, 40, 32
    assert steps < new
    prompt = torch.randint(0, 32000, (b, ctx - 64), device="cuda")
    decs = {}
    for dtype in ("bf16", "fp8"):
        dec = CapturedLlamaDecoder(model, max_batch=b, max_seq_len=ctx,
                                   kv_cache_dtype=dtype)
        dec.generate(prompt, new)  # prefill + capture
        decs[dtype] = dec
        per_layer = sum(t.numel() * t.element_size() for t in dec.caches[0][:-1])
        print(f"{dtype}: cache bytes per layer {per_layer} "
              f"({per_layer / 2 ** 20:.1f} MiB)", flush=True)
    # replays advance the position: rewind before each timed run so that both
    # versions always decode at the same context
    def rewound(dec):
        first = dec.out_tokens[:, 0:1].clone()

        def run():
            dec._reset_to(ctx - 64, first)
            for _ in range(steps):
                dec.graph.replay()
        return run

    t = _alternate({n: rewound(d) for n, d in decs.items()}, 1, args.rounds)
    for n, x in t.items():
        x = [v / steps for v in x]
        print(f"{n}: captured step {statistics.median(x):.1f} us "
              f"({min(x):.1f}..{max(x):.1f}), b{b} ctx{ctx}")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--no-kernel", action="store_true")
    args = p.parse_args()
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    with torch.no_grad():
        if not args.no_kernel:
            kernel_level(args)
        if args.e2e:
            end_to_end(args)
