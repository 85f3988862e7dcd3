#!/usr/bin/env python3
"""Swin WindowAttention A/B: the fused window-attention kernels
(fused_window_attention=True) vs the materialized path (bmm -> +bias -> +mask
-> fp32 softmax -> bmm -> transpose copy), training forward + backward of the
layer, at the four stage shapes of configs/swin_cifar_pretrain.py-style Swin-T
at batch 64: (B_, H) = (4096, 3), (1024, 6), (256, 12), (64, 24), N = 49,
C = 32 H, with and without the shift mask.  Routes are timed alternately,
several rounds each; a timed window holds as many steps as fill --window-ms
(counted per route and shape from a calibration run), so the short stages
are not timed over a few milliseconds.  Which route ran is asserted.

Usage (GPU box): python tools/swin_window_bench.py [--window-ms 500] [--rounds 5]
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def _timed(fn, steps):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return ((time.perf_counter() - t0) * 1e3 / steps,
            torch.cuda.max_memory_allocated() - base)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--window-ms", type=float, default=500.0)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available(), "swin_window_bench needs a GPU"

    import libai_amd.models.swin_transformer as S
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    torch.manual_seed(0)
    calls = [0]
    orig = S.window_attention

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)

    S.window_attention = counted

    ws, n = 7, 49
    print(f"# Swin WindowAttention fwd+bwd, batch {args.batch}, N {n}, bf16; "
          f"{args.rounds} rounds of about {args.window_ms:.0f} ms per route, "
          f"alternating\n")
    print("| B_ | H | mask | materialized ms (min..max) | fused ms (min..max) | "
          "speed-up | steps per window mat. / fused | peak MB mat. -> fused |")
    print("|---|---|---|---|---|---|---|---|")
    for stage, heads in enumerate((3, 6, 12, 24)):
        res = 56 >> stage
        nw = (res // ws) ** 2
        b_ = args.batch * nw
        dim = 32 * heads
        base = S.WindowAttention(dim, ws, heads).cuda().bfloat16().train()
        fused = S.WindowAttention(dim, ws, heads,
                                  fused_window_attention=True).cuda().bfloat16().train()
        fused.load_state_dict(base.state_dict())
        x = torch.randn(b_, n, dim, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        g = torch.randn_like(x)
        for masked in (False, True):
            mask = None
            if masked:
                mask = torch.where(torch.rand(nw, n, n, device="cuda") < 0.3, -100.0, 0.0)

            def step(mod):
                def fn():
                    mod.zero_grad(set_to_none=True)
                    x.grad = None
                    mod(x, mask=mask).backward(g)
                return fn

            routes = {"mat": step(base), "fused": step(fused)}
            c0 = calls[0]
            routes["mat"]()
            assert calls[0] == c0, "the default layer must not call the fused op"
            routes["fused"]()
            assert calls[0] == c0 + 1, "the flagged layer must call the fused op"
            for fn in routes.values():
                for _ in range(3):
                    fn()
            steps = {k: max(20, int(args.window_ms / _timed(fn, 20)[0]) + 1)
                     for k, fn in routes.items()}
            ms = {k: [] for k in routes}
            peak = {k: 0 for k in routes}
            for _ in range(args.rounds):
                for k, fn in routes.items():
                    t, pk = _timed(fn, steps[k])
                    ms[k].append(t)
                    peak[k] = max(peak[k], pk)
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(f"| {b_} | {heads} | {'yes' if masked else 'no'} | "
                  f"{med['mat']:.3f} ({min(ms['mat']):.3f}..{max(ms['mat']):.3f}) | "
                  f"{med['fused']:.3f} ({min(ms['fused']):.3f}..{max(ms['fused']):.3f}) | "
                  f"{med['mat'] / med['fused']:.2f}x | "
                  f"{steps['mat']} / {steps['fused']} | "
                  f"{peak['mat'] / 2**20:.0f} -> {peak['fused'] / 2**20:.0f} |",
                  flush=True)
        del base, fused, x, g


if __name__ == "__main__":
    main()
