#!/usr/bin/env python3
"""Record the bits of the flash-attention training kernels as fixtures.

Run ONCE on a GPU, on the commit whose arithmetic is to be pinned, *before*
the kernels are changed:

    python tools/make_flash_golden.py            # refuses to overwrite
    python tools/make_flash_golden.py --force    # re-record on purpose
    python tools/make_flash_golden.py --only-missing   # new cases only

`tests/gpu/test_flash_staging_gpu.py` rebuilds the same inputs through
`cases()` / `make_inputs()` and asserts that the build under test reproduces
the recorded outputs bit for bit.  The inputs are pure functions of numpy's
legacy `RandomState` streams (stable across numpy versions), made on the CPU
and moved to the device, so only outputs are stored:
`tests/golden/flash_stage_<case>_d<D>.npz`, holding the raw bit patterns of O,
dQ, dK, dV (bf16 as uint16) and lse (fp32 as uint32); forward-only cases hold
O and lse.  The relative-position table's gradient is not recorded: its sum
goes through atomics and has no fixed bits.

The cases are the shapes at which a K/V staging loop can go wrong: one round
of 128 keys, a last round of 8 valid rows, three ragged rounds, Sq != Sk,
staged rows past kv_len, a loop that starts at a later round (window, packed
documents), the table staging between the same barriers (rel_bias), dropout,
and a ragged key count behind a query offset.
"""

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DROP_SEED = (1 << 61) + 0xDEADBEEF

# name, then: b, h, hkv, sq, sk, causal and the options of the case
_BASE = dict(b=1, h=2, hkv=2, causal=True, p=0.0, kv_len=None, window=0, docs=None,
             rel_bias=False, q_offset=0, backward=True)
_SHAPES = (
    ("one_round", dict(sq=128, sk=128)),
    ("tail8_gqa", dict(sq=136, sk=136, h=4)),
    ("ragged3", dict(sq=264, sk=264)),
    ("cross", dict(sq=40, sk=200, causal=False)),
    ("kv_len", dict(b=2, sq=264, sk=264, kv_len=(264, 97))),
    ("window40", dict(sq=384, sk=384, window=40)),
    ("docs", dict(sq=384, sk=384, docs=(100, 150, 134))),
    ("rel_bias", dict(sq=264, sk=264, rel_bias=True)),
    ("dropout", dict(sq=264, sk=264, p=0.1)),
    ("offset", dict(sq=8, sk=117, q_offset=109, backward=False)),
)
# D = 128 walks other tile sizes (32-key dQ tiles, sixteen chunks per forward
# round); the cases kept for it are the ragged, Sq != Sk, table and offset ones
_D128 = ("tail8_gqa", "ragged3", "cross", "rel_bias", "offset")


def cases():
    """yields one dict per case: name, d and the fields of _BASE / _SHAPES"""
    for i, (name, over) in enumerate(_SHAPES):
        for d in (64, 128):
            if d == 128 and name not in _D128:
                continue
            yield dict(_BASE, **over, d=d, seed=100 + i, name=f"flash_stage_{name}_d{d}")


def _randn(rs, shape, dtype=torch.bfloat16):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dtype)


def make_inputs(c):
    """CPU tensors of case c: q, k, v, dout [B, S, H, D] bf16, and kv_len
    (int32), table (fp32 [H, Sq + Sk - 1]), doc_start / doc_end (int32
    [B, S]) or None."""
    rs = np.random.RandomState(c["seed"])
    b, h, hkv, sq, sk, d = (c[x] for x in ("b", "h", "hkv", "sq", "sk", "d"))
    t = {"q": _randn(rs, (b, sq, h, d)), "k": _randn(rs, (b, sk, hkv, d)),
         "v": _randn(rs, (b, sk, hkv, d)), "dout": _randn(rs, (b, sq, h, d)),
         "kv_len": None, "table": None, "doc_start": None, "doc_end": None}
    if c["kv_len"] is not None:
        t["kv_len"] = torch.tensor(c["kv_len"], dtype=torch.int32)
        # loss-mask contract: padded QUERY rows never reach the loss
        qmask = torch.arange(sq)[None, :] < t["kv_len"][:, None]
        t["dout"] = t["dout"] * qmask[:, :, None, None].to(t["dout"].dtype)
    if c["rel_bias"]:
        t["table"] = _randn(rs, (h, sq + sk - 1), torch.float32) * 0.5
    if c["docs"] is not None:
        sys.path.insert(0, ROOT)
        from libai_amd.data.packing import doc_bounds_from_lengths

        ds, de = doc_bounds_from_lengths(list(c["docs"]), sq)[:2]
        t["doc_start"] = ds.to(torch.int32).repeat(b, 1).contiguous()
        t["doc_end"] = de.to(torch.int32).repeat(b, 1).contiguous()
    return t


def scale_of(c):
    return 1.0 / float(np.sqrt(c["d"]))


def run_case(ext, c, t, device="cuda"):
    """-> dict of device tensors: o, lse and, for a backward case, dq, dk, dv
    (and dtable with a rel_bias table)"""
    g = {k: (v.to(device) if v is not None else None) for k, v in t.items()}
    seed = DROP_SEED if c["p"] > 0 else 0
    o, lse = ext.flash_fwd(g["q"], g["k"], g["v"], scale_of(c), c["p"], seed,
                           c["causal"], g["kv_len"], None, c["window"], g["table"],
                           g["doc_start"], g["doc_end"], c["q_offset"])
    res = {"o": o, "lse": lse}
    if c["backward"]:
        out = ext.flash_bwd(g["q"], g["k"], g["v"], o, g["dout"], lse, scale_of(c),
                            c["p"], seed, c["causal"], None, g["kv_len"], None,
                            c["window"], g["table"], g["doc_start"], g["doc_end"])
        res.update(dq=out[0], dk=out[1], dv=out[2])
        if c["rel_bias"]:
            res["dtable"] = out[3]
    return res


def bits(x):
    """raw bit pattern of a bf16 / fp32 tensor as a numpy uint16 / uint32 array"""
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


RECORDED = ("o", "lse", "dq", "dk", "dv")


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
        sys.exit("make_flash_golden: needs a GPU (the fixtures record its arithmetic)")
    todo = list(cases())
    existing = [c["name"] for c in todo if os.path.exists(golden_path(c["name"]))]
    if args.only_missing:
        todo = [c for c in todo if c["name"] not in existing]
        existing = []
    if existing and not args.force:
        sys.exit("make_flash_golden: fixtures exist (%s, ...); they pin the parent's "
                 "arithmetic -- pass --force to re-record" % existing[0])
    os.makedirs(GOLDEN, exist_ok=True)
    for c in todo:
        res = run_case(ext(), c, make_inputs(c))
        path = golden_path(c["name"])
        np.savez_compressed(path, **{k: bits(res[k]) for k in RECORDED if k in res})
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
