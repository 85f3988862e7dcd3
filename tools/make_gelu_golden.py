#!/usr/bin/env python3
"""Record the bits of bias_gelu (forward, backward, bias gradient) as fixtures.

Run ONCE on a GPU, on the commit whose arithmetic is to be pinned, *before*
the kernel is changed:

    python tools/make_gelu_golden.py            # refuses to overwrite
    python tools/make_gelu_golden.py --force    # re-record on purpose
    python tools/make_gelu_golden.py --only-missing   # new cases only

`tests/gpu/test_elementwise_bits_gpu.py` rebuilds the same inputs through
`cases()` and asserts that the build under test reproduces the recorded
outputs bit for bit.  The inputs are pure functions of fixed constants and
numpy's legacy `RandomState` streams (stable across numpy versions), so only
outputs are stored: `tests/golden/bias_gelu_<dtype>_<bias>_<what>.npz`, each
holding one array of raw bit patterns (uint16 for bf16, uint32 for fp32) and,
for the backward of a biased case, the bias gradient's bits.
"""

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
W = 8192

# sums x + b with these fall between bf16 points for most x; 2^-9 and 2^-20
# stay exact additions that land on or next to rounding ties
BIAS_VALUES = (0.3, -1.7, 2.0 ** -9, -(2.0 ** -20), 3.1415927, -0.0078125 * 1.5,
               117.0, -2.0 ** -126)


def _bits_dtype(dtype):
    return torch.int16 if dtype == torch.bfloat16 else torch.int32


def bf16_grid():
    """all 65536 bf16 bit patterns, in order, as a [8, 8192] bf16 tensor"""
    bits = np.arange(65536, dtype=np.uint16).view(np.int16)
    return torch.from_numpy(bits.copy()).view(torch.bfloat16).view(8, W)


def make_x(dtype):
    if dtype == torch.bfloat16:
        return bf16_grid()
    rs = np.random.RandomState(1234)
    seeded = torch.from_numpy((rs.standard_normal(65536) * 3.0).astype(np.float32))
    return torch.cat([seeded.view(8, W), bf16_grid().float()], 0)


def make_bias(dtype):
    return torch.tensor(BIAS_VALUES, dtype=torch.float32).repeat(W // 8).to(dtype)


def make_dy(dtype, kind, shape):
    if kind == "ones":
        return torch.ones(shape, dtype=dtype)
    rs = np.random.RandomState(4321)
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dtype)


# Tall cases: width 8, so that the launch has 4096 row-blocks and a thread
# walks several rows (2 each at 8192 rows; 4 or 3 at 12293): the row loop and
# the in-thread order of the bias-gradient sum, which the wide cases above
# (one row per thread) never reach.
TALL_W = 8
TALL = (("bf16", torch.bfloat16, 8192), ("bf16", torch.bfloat16, 12293),
        ("f32", torch.float32, 12293))


def make_tall_x(dtype, rows):
    """the bf16 grid, cycled, with inf / NaN patterns mapped to finite ones
    (exponent bit 6 cleared) so that every column's gradient sum is finite;
    fp32 adds seeded low bits below the bf16 mantissa"""
    n = rows * TALL_W
    bits = (np.arange(n, dtype=np.int64) * 40503 % 65536).astype(np.uint16)
    nonfinite = (bits & 0x7F80) == 0x7F80
    bits = np.where(nonfinite, bits & ~np.uint16(0x2000), bits).astype(np.uint16)
    x = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)
    if dtype == torch.float32:
        low = np.random.RandomState(99).randint(0, 1 << 16, n).astype(np.uint32)
        wide = (bits.astype(np.uint32) << 16) | low
        x = torch.from_numpy(wide.view(np.int32).copy()).view(torch.float32)
    return x.view(rows, TALL_W)


def tall_cases():
    for dname, dtype, rows in TALL:
        x = make_tall_x(dtype, rows)
        bias = torch.tensor(BIAS_VALUES, dtype=torch.float32).to(dtype)
        yield f"bias_gelu_{dname}_tall{rows}_fwd", dtype, x, bias, None
        yield (f"bias_gelu_{dname}_tall{rows}_bwd_rand", dtype, x, bias,
               make_dy(dtype, "rand", (rows, TALL_W)))


def cases():
    """yields (name, dtype, x, bias or None, dy or None); dy None = forward"""
    for dname, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        x = make_x(dtype)
        for bname, bias in (("nobias", None), ("bias", make_bias(dtype))):
            yield f"bias_gelu_{dname}_{bname}_fwd", dtype, x, bias, None
            for kind in ("ones", "rand"):
                yield (f"bias_gelu_{dname}_{bname}_bwd_{kind}", dtype, x, bias,
                       make_dy(dtype, kind, tuple(x.shape)))
    yield from tall_cases()


def run_case(ext, x, bias, dy, device="cuda"):
    """-> dict of int tensors (raw bits) on the CPU: `out`, and `db` if any"""
    xd = x.to(device)
    bd = bias.to(device) if bias is not None else None
    bits = _bits_dtype(x.dtype)
    if dy is None:
        return {"out": ext.bias_gelu_fwd(xd, bd).view(bits).cpu()}
    dx, db = ext.bias_gelu_bwd(xd, bd, dy.to(device), bd is not None)
    res = {"out": dx.view(bits).cpu()}
    if db is not None:
        res["db"] = db.view(bits).cpu()
    return res


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--force", action="store_true",
                    help="overwrite fixtures that already exist")
    ap.add_argument("--only-missing", action="store_true",
                    help="record the cases that have no fixture yet, touch no other")
    args = ap.parse_args()

    sys.path.insert(0, ROOT)
    from libai_amd.ops._ext import ext

    if not torch.cuda.is_available():
        sys.exit("make_gelu_golden: needs a GPU (the fixtures record its arithmetic)")
    todo = list(cases())
    existing = [n for n, *_ in todo if os.path.exists(golden_path(n))]
    if args.only_missing:
        todo = [c for c in todo if c[0] not in existing]
        existing = []
    if existing and not args.force:
        sys.exit("make_gelu_golden: fixtures exist (%s, ...); they pin the parent's "
                 "arithmetic -- pass --force to re-record" % existing[0])
    os.makedirs(GOLDEN, exist_ok=True)
    for name, _dtype, x, bias, dy in todo:
        res = run_case(ext(), x, bias, dy)
        np.savez_compressed(golden_path(name),
                            **{k: v.numpy() for k, v in res.items()})
        print(f"wrote {golden_path(name)} ({os.path.getsize(golden_path(name))} bytes)")


if __name__ == "__main__":
    main()
