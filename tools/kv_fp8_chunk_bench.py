#!/usr/bin/env python3
"""Multi-token steps on the FP8 KV cache (profiles/kv_fp8_chunk.md).

Kernel level: one T-token flash_decode_attn_fp8 call (T = 2, 4, 8) against one
single-token call and against T single-token calls in a row, batch 32, G = 4,
head size 128, contexts 1024 and 4096; all versions alternated inside one
process, device events around runs of --iters calls, --rounds rounds per
version (median and min..max reported).
End to end (--e2e): a speculate(K = 4) step of the Llama-1B-GQA bench model on
ContinuousLlamaDecoder(fp8) at b32 ctx1024 against K + 1 replays of its captured
single-token step, both rewound to the same positions before every run.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from kv_fp8_bench import _alternate  # noqa: E402  (tools/ is on sys.path)

TOKENS = (2, 4, 8)


def _cell(xs):
    return f"{statistics.median(xs):.1f} ({min(xs):.1f}..{max(xs):.1f})"


def kernel_level(args):
    from libai_amd.ops.attention import flash_decode_attn_fp8

    b, h, kvh, d = 32, 32, 8, 128
    sm = d ** -0.5
    print("| ctx | T | 1 single us (min..max) | T singles us | one T-token call us | "
          "T-token / single | T singles / T-token |")
    print("|---|---|---|---|---|---|---|")
    for ctx in (1024, 4096):
        torch.manual_seed(0)
        q = torch.randn(b, h, max(TOKENS), d, device="cuda", dtype=torch.bfloat16)
        caches = []
        for _ in range(2):
            x = torch.randn(b, kvh, ctx, d, device="cuda")
            scale = x.abs().amax(-1) / 448.0
            c8 = (x / scale[..., None]).clamp(-448, 448)
            caches += [c8.to(torch.float8_e4m3fn).view(torch.uint8), scale]
        k8, ks, v8, vs = caches
        kv_len = torch.full((b,), ctx, dtype=torch.int32, device="cuda")

        def call(t0, t1):
            return flash_decode_attn_fp8(q[:, :, t0:t1], k8, v8, ks, vs, sm,
                                         kv_len=kv_len)

        def singles(t):
            for i in range(t):
                call(i, i + 1)

        fns = {"single": lambda: call(0, 1)}
        for t in TOKENS:
            fns[f"chunk{t}"] = lambda t=t: call(0, t)
            fns[f"singles{t}"] = lambda t=t: singles(t)
        times = _alternate(fns, args.iters, args.rounds)
        one = statistics.median(times["single"])
        for t in TOKENS:
            ch = statistics.median(times[f"chunk{t}"])
            sg = statistics.median(times[f"singles{t}"])
            print(f"| {ctx} | {t} | {_cell(times['single'])} | "
                  f"{_cell(times[f'singles{t}'])} | {_cell(times[f'chunk{t}'])} | "
                  f"{ch / one:.2f}x | {sg / ch:.2f}x |", flush=True)


def end_to_end(args):
    from libai_amd.inference.captured_decode import ContinuousLlamaDecoder
    from libai_amd.models import LlamaForCausalLM

    torch.manual_seed(0)
    model = LlamaForCausalLM(
        hidden_layers=16, vocab_size=32000, hidden_size=2048,
        intermediate_size=5504, num_attention_heads=16,
        num_key_value_heads=4, max_position_embeddings=4096,
    ).to(torch.bfloat16).cuda().eval()
    b, ctx, k = 32, 1024, 4
    dec = ContinuousLlamaDecoder(model, max_batch=b, max_seq_len=ctx,
                                 kv_cache_dtype="fp8")
    for slot in range(b):
        dec.add_request(slot, torch.randint(0, 32000, (ctx - 64,), device="cuda"))
    dec.step(1)  # captures the single-token step
    state = (dec.pos, dec.kv32, dec.slot_step, dec.static_tok)
    snap = [t.clone() for t in state]
    draft = torch.randint(0, 32000, (b, k), device="cuda")

    def rewound(fn):
        def run():  # both versions always start from the same positions
            for t, s in zip(state, snap):
                t.copy_(s)
            fn()
        return run

    def replays():
        for _ in range(k + 1):
            dec.graph.replay()

    t = _alternate({"speculate": rewound(lambda: dec.speculate(draft)),
                    "replays": rewound(replays)}, args.e2e_iters, args.rounds)
    print(f"speculate(K={k}) step: {_cell(t['speculate'])} us; {k + 1} captured "
          f"replays: {_cell(t['replays'])} us; b{b} ctx{ctx}; replays / speculate "
          f"{statistics.median(t['replays']) / statistics.median(t['speculate']):.2f}x")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--e2e-iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--e2e", action="store_true")
    p.add_argument("--no-kernel", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv_fp8_chunk_bench.py times GPU kernels: no GPU found")
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    with torch.no_grad():
        if not args.no_kernel:
            kernel_level(args)
        if args.e2e:
            end_to_end(args)
