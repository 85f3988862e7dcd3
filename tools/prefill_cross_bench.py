#!/usr/bin/env python3
"""A/B of the opt-in flash routes against the same layer with the flag off
(the flag-off layer is the code every caller ran before the flags existed).

prompt: a Llama-7B-shaped attention layer (32 heads, D 128, b 1; also the GQA
form with 8 kv heads), prompt pass with use_cache at S in {512, 2048, 4096}.
chunk: the same layers, a step of Sq in {2, 16, 128, 512} tokens on 4096
cached keys.
sweep: the chunk case at Sq in {16, 128} on {256, 512, 1024, 2048} cached keys.
cross: a T5-base decoder cross-attention (hidden 768, 12 heads), forward +
backward at the shapes of configs/t5_pretrain.py (b 16, 114 queries, 512
keys), with and without dropout.

Device events around INNER calls; WARM warm-up calls per variant, then REPS
rounds that alternate the variants; median and min..max of the per-round
means.  Peak memory is torch.cuda.max_memory_allocated over one call, minus
what was allocated before it.  One JSON line per case.

Usage (GPU box): python tools/prefill_cross_bench.py [all|prompt|chunk|sweep|cross]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from libai_amd.utils import distributed as du

du.setup_dist_util({})
dev = "cuda"
REPS, INNER, WARM = 7, 10, 3
out = []


def timed(fns, inner=INNER):
    """fns: dict name -> callable; returns name -> (median ms, min, max), peak MiB"""
    res, mem = {n: [] for n in fns}, {}
    for n, f in fns.items():
        for _ in range(WARM):
            f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f()
        torch.cuda.synchronize()
        mem[n] = (torch.cuda.max_memory_allocated() - base) / 2**20
    for _ in range(REPS):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            res[n].append(e0.elapsed_time(e1) / inner)
    return {n: (statistics.median(v), min(v), max(v), mem[n]) for n, v in res.items()}


def report(tag, r):
    row = {"case": tag}
    for n, (med, lo, hi, mem) in r.items():
        row[n] = dict(ms=round(med, 4), min=round(lo, 4), max=round(hi, 4),
                      peak_mib=round(mem, 1))
    out.append(row)
    print(json.dumps(row), flush=True)


def llama_pair(kvh):
    from libai_amd.models.llama import LlamaAttention

    init = torch.nn.init.xavier_normal_
    torch.manual_seed(0)
    off = LlamaAttention(4096, 32, 8192, init, init, num_key_value_heads=kvh)
    on = LlamaAttention(4096, 32, 8192, init, init, num_key_value_heads=kvh,
                        flash_prefill=True)
    off = off.to(dev, torch.bfloat16).eval()
    on = on.to(dev, torch.bfloat16).eval()
    on.load_state_dict(off.state_dict())
    return off, on


which = sys.argv[1] if len(sys.argv) > 1 else "all"
# the chunk tables are what the layers' gate (ops.attention.flash_chunk_pays)
# was taken from: measure the flash route itself, gated shapes included
import libai_amd.models.llama as _llama

_llama.flash_chunk_pays = lambda *a: True
with torch.no_grad():
    for kvh in (32, 8):
        off, on = llama_pair(kvh)
        if which in ("all", "prompt"):
            for s in (512, 2048, 4096):
                x = torch.randn(1, s, 4096, device=dev, dtype=torch.bfloat16)
                r = timed({"off": lambda: off(x, use_cache=True),
                           "on": lambda: on(x, use_cache=True)})
                a = off(x, use_cache=True)[0].float()
                b = on(x, use_cache=True)[0].float()
                report(f"prompt kvh{kvh} S{s} relerr "
                       f"{((a - b).abs().max() / a.abs().max()).item():.2e}", r)
        if which in ("all", "chunk"):
            past = tuple(torch.randn(1, kvh, 4096, 128, device=dev, dtype=torch.bfloat16)
                         for _ in range(2))
            for sq in (2, 16, 128, 512):
                x = torch.randn(1, sq, 4096, device=dev, dtype=torch.bfloat16)
                r = timed({"off": lambda: off(x, past_key_value=past, use_cache=True),
                           "on": lambda: on(x, past_key_value=past, use_cache=True)})
                report(f"chunk kvh{kvh} Sq{sq} on 4096", r)
        if which == "sweep":  # where the chunk route starts to lose: fewer keys
            for sk in (256, 512, 1024, 2048):
                past = tuple(torch.randn(1, kvh, sk, 128, device=dev,
                                         dtype=torch.bfloat16) for _ in range(2))
                for sq in (16, 128):
                    x = torch.randn(1, sq, 4096, device=dev, dtype=torch.bfloat16)
                    r = timed({"off": lambda: off(x, past_key_value=past, use_cache=True),
                               "on": lambda: on(x, past_key_value=past, use_cache=True)})
                    report(f"chunk kvh{kvh} Sq{sq} on {sk}", r)
        del off, on

if which in ("all", "cross"):
    from libai_amd.layers import MultiheadAttention
    from libai_amd.models.t5_model import cross_attn_mask

    for p in (0.1, 0.0):
        torch.manual_seed(0)
        off = MultiheadAttention(768, 12, is_cross_attention=True,
                                 attention_dropout_prob=p, output_dropout_prob=p)
        on = MultiheadAttention(768, 12, is_cross_attention=True,
                                attention_dropout_prob=p, output_dropout_prob=p,
                                flash_cross_attention=True)
        off = off.to(dev, torch.bfloat16).train()
        on = on.to(dev, torch.bfloat16).train()
        on.load_state_dict(off.state_dict())
        b, sq, sk = 16, 114, 512
        x = torch.randn(b, sq, 768, device=dev, dtype=torch.bfloat16, requires_grad=True)
        enc = torch.randn(b, sk, 768, device=dev, dtype=torch.bfloat16,
                          requires_grad=True)
        mask = cross_attn_mask(torch.ones(b, sq, dtype=torch.uint8, device=dev),
                               torch.ones(b, sk, dtype=torch.uint8, device=dev))
        g = torch.randn(b, sq, 768, device=dev, dtype=torch.bfloat16)

        def step(layer):
            def f():
                y = layer(x, encoder_states=enc, attention_mask=mask)
                y.backward(g)
                x.grad = enc.grad = None
            return f

        r = timed({"off": step(off), "on": step(on)})
        report(f"t5 cross fwd+bwd b16 Sq114 Sk512 p{p}", r)
