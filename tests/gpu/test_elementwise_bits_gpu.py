"""Bit-level checks of the elementwise kernels (run on MI355X).

* the bf16 round of `common.h` (hardware convert) against torch's
  round-to-nearest-even, through `bias_dropout_add` at p = 0;
* `bias_gelu` forward / backward / bias gradient against bits recorded from
  the kernel as it was before its division and its bf16 round were rewritten
  (`tools/make_gelu_golden.py` -> `tests/golden/bias_gelu_*.npz`);
* the 16-byte path of `adamw_kernel` / `l2norm_sq_kernel` against the scalar
  path, by placing the same parameter at an aligned and at an odd offset.
"""

import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module", autouse=True)
def _setup():
    from libai_amd.utils import distributed as du

    du.setup_dist_util({})
    from libai_amd.ops._ext import has_ext

    assert has_ext(), "HIP extension must be built+loaded on the GPU box"
    yield


def _ext():
    from libai_amd.ops._ext import ext

    return ext()


# ---------------------------------------------------------------------------
# bf16 round
# ---------------------------------------------------------------------------
def _all_bf16():
    bits = np.arange(65536, dtype=np.uint16).view(np.int16)
    return torch.from_numpy(bits.copy()).view(torch.bfloat16)


# res = sign * mant * 2^(e + shift), e the exponent of x (bf16 ulp = 2^(e-7)):
# half an ulp (a tie: rounds to the even neighbour, so both parities of the
# kept bit occur over the grid), a quarter (just below) and three quarters
# (just above).  At the largest exponent the tie rounds up into infinity; at
# the smallest ones the residual is itself subnormal or rounds to zero, which
# is fine: the reference is formed from the residual as it is.
_RESIDUALS = [(s, m, sh) for s in (1.0, -1.0) for m, sh in ((1.0, -8), (1.0, -9), (3.0, -10))]


@pytest.mark.parametrize("sign,mant,shift", _RESIDUALS)
def test_bf16_round_is_nearest_even(sign, mant, shift):
    from libai_amd.ops.fused_bias import bias_dropout_add

    x = _all_bf16()
    xf = x.float()
    finite = torch.isfinite(xf)
    # exponent e with 2^e <= |x| < 2^(e+1); zero, subnormals, inf, NaN: -126
    _, ex = torch.frexp(torch.where(finite & (xf != 0), xf, torch.ones_like(xf)))
    e = torch.where(finite & (xf.abs() >= 2.0 ** -126), ex - 1, torch.full_like(ex, -126))
    res = torch.ldexp(torch.full_like(xf, sign * mant), e + shift).to(torch.bfloat16)
    # without a bias the kernel adds a zero one: (x + 0) + res.  That is
    # x + res except in the sign of one zero, -0 + -0 (0x8000 with a residual
    # that underflowed to -0), which has nothing to do with the rounding.
    ref = ((xf + 0.0) + res.float()).to(torch.bfloat16)
    plain = (xf + res.float()).to(torch.bfloat16)
    differs = ref.view(torch.int16) != plain.view(torch.int16)
    assert not differs[~torch.isnan(ref)].any() or (
        differs.nonzero().view(-1).tolist() == [0x8000] and sign < 0
        and plain[0x8000].item() == 0 and ref[0x8000].item() == 0)

    out = bias_dropout_add(x.view(8, 8192).cuda(), None, res.view(8, 8192).cuda(),
                           p=0.0).cpu().view(-1)
    nan = torch.isnan(ref)
    # the sums are exact in fp32 where nothing underflows: make sure the grid
    # really exercises ties (exact halves), in both parities
    exact = xf.double() + res.double()
    assert (exact[finite] == (xf + res.float())[finite].double()).all()
    assert torch.equal(torch.isnan(out), nan)
    bad = (out.view(torch.int16) != ref.view(torch.int16)) & ~nan
    assert not bad.any(), [
        (hex(i), hex(res.view(torch.int16)[i].item() & 0xFFFF),
         hex(out.view(torch.int16)[i].item() & 0xFFFF),
         hex(ref.view(torch.int16)[i].item() & 0xFFFF))
        for i in bad.nonzero().view(-1).tolist()[:8]]
    if shift == -8:
        tie_up = (ref.float().abs() > exact.abs()) & finite & ~nan
        tie_down = (ref.float().abs() < exact.abs()) & finite & ~nan
        assert tie_up.sum() > 10000 and tie_down.sum() > 10000
        assert torch.isinf(ref[finite]).any(), "the tie at the top exponent overflows"


# ---------------------------------------------------------------------------
# bias_gelu against the recorded bits
# ---------------------------------------------------------------------------
def _golden_tool():
    spec = importlib.util.spec_from_file_location(
        "make_gelu_golden", os.path.join(ROOT, "tools", "make_gelu_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TOOL = _golden_tool()
_CASES = {name: rest for name, *rest in _TOOL.cases()}


def _as_float(bits, dtype):
    t = torch.from_numpy(bits)
    return t.view(dtype).float()


def _assert_same_bits(got_bits, want_bits, finite_in, dtype, what):
    """bit-equal where the input is finite; elsewhere NaN stays NaN and an
    infinity keeps its sign"""
    got_bits, want_bits = got_bits.numpy(), want_bits
    neq = (got_bits != want_bits) & finite_in.numpy()
    assert not neq.any(), (
        f"{what}: {int(neq.sum())} outputs of finite inputs differ, first at "
        f"{np.argwhere(neq)[0].tolist()}: got {got_bits[neq][0]:#x}, "
        f"recorded {want_bits[neq][0]:#x}")
    g, w = _as_float(got_bits, dtype), _as_float(want_bits, dtype)
    rest = ~finite_in
    assert torch.equal(torch.isnan(g)[rest], torch.isnan(w)[rest]), what
    inf = torch.isinf(w) & rest
    assert torch.equal(torch.isinf(g) & rest, inf), what
    assert torch.equal(g[inf], w[inf]), what


@pytest.mark.parametrize("name", sorted(_CASES))
def test_bias_gelu_reproduces_recorded_bits(name):
    dtype, x, bias, dy = _CASES[name]
    want = np.load(_TOOL.golden_path(name))
    got = _TOOL.run_case(_ext(), x, bias, dy)

    xin = x.float() + (bias.float() if bias is not None else 0.0)
    finite_in = torch.isfinite(x.float()) & torch.isfinite(xin)
    _assert_same_bits(got["out"], want["out"], finite_in, dtype, name)

    assert ("db" in got) == ("db" in want.files)
    if "db" in got:
        # the partial layout and the summation order are unchanged: equal
        # bits in every column whose rows are all finite (NaN != NaN
        # otherwise), the same class in the columns that hold inf / NaN rows
        # In the tall cases (width 8, 4096 row-blocks) a thread sums 2 to 4
        # rows in order and every column is finite: they pin the row loop's
        # indexing, its x / dy pairing and the in-thread summation order.
        col_finite = finite_in.all(0)
        assert col_finite.all() if "tall" in name else col_finite.sum() >= 8192 - 128
        _assert_same_bits(got["db"], want["db"], col_finite, dtype, name + " dbias")


# ---------------------------------------------------------------------------
# AdamW / l2norm: 16-byte path == scalar path
# ---------------------------------------------------------------------------
_SIZES = [1, 7, 8, 9, 65535, 65536, 65537, 3 * 65536 + 5]
_STREAMS = ("param", "master", "grad", "m", "v")
_HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, grad_scale=0.5)


def _place(src, offset):
    """a copy of `src` at element `offset` of a fresh 16-byte-aligned buffer"""
    buf = torch.empty(src.numel() + 16, dtype=src.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + src.numel()]
    view.copy_(src)
    assert (view.data_ptr() % 16 == 0) == (offset * src.element_size() % 16 == 0)
    return view


def _chunks(ptrs, n, esizes):
    chunk = _ext().adamw_chunk_elems()
    rows = []
    for s in range(0, n, chunk):
        rows.append([p + s * e if p else 0 for p, e in zip(ptrs, esizes)] + [min(chunk, n - s)])
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


_ADAM_INPUTS = {}


def _adam_inputs(bf16, n):
    """seeded CPU state of one parameter and three gradients, made once"""
    key = (bf16, n)
    if key not in _ADAM_INPUTS:
        g = torch.Generator().manual_seed(1000 + n)
        master = torch.randn(n, generator=g)
        gdt = torch.bfloat16 if bf16 else torch.float32
        grads = [(torch.randn(n, generator=g) * (10.0 ** -k)).to(gdt) for k in range(3)]
        _ADAM_INPUTS[key] = (master, grads)
    return _ADAM_INPUTS[key]


def _run_adamw(bf16, n, offsets):
    """three updates with the streams at the given element offsets; returns
    the state after each as CPU tensors (p16 or None, master, m, v)"""
    master0, grads = _adam_inputs(bf16, n)
    master = _place(master0, offsets["master"])
    m = _place(torch.zeros(n), offsets["m"])
    v = _place(torch.zeros(n), offsets["v"])
    grad = _place(grads[0], offsets["grad"])
    p16 = _place(master0.to(torch.bfloat16), offsets["param"]) if bf16 else None
    ptrs = [p16.data_ptr() if bf16 else 0, master.data_ptr(), grad.data_ptr(),
            m.data_ptr(), v.data_ptr()]
    gsz = 2 if bf16 else 4
    desc = _chunks(ptrs, n, [2, 4, gsz, 4, 4])
    states = []
    h = _HYPER
    for t in range(1, 4):
        grad.copy_(grads[t - 1])
        _ext().adamw_step(desc, bf16, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"],
                          1 - h["beta1"] ** t, 1 - h["beta2"] ** t, h["grad_scale"])
        states.append(tuple(None if s is None else s.cpu().clone()
                            for s in (p16, master, m, v)))
    return states


def _assert_states_equal(a, b):
    for t, (sa, sb) in enumerate(zip(a, b), 1):
        for name, ta, tb in zip(("p16", "master", "m", "v"), sa, sb):
            if ta is None:
                assert tb is None
                continue
            assert torch.isfinite(ta.float()).all()
            assert torch.equal(ta, tb), f"step {t}: {name} differs between the paths"


_ALIGNED = dict.fromkeys(_STREAMS, 0)
_ADAM_ALIGNED = {}


def _aligned_run(bf16, n):
    key = (bf16, n)
    if key not in _ADAM_ALIGNED:
        _ADAM_ALIGNED[key] = _run_adamw(bf16, n, _ALIGNED)
    return _ADAM_ALIGNED[key]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16_master", "fp32_native"])
@pytest.mark.parametrize("n", _SIZES)
def test_adamw_vector_path_equals_scalar_path(bf16, n):
    vec = _aligned_run(bf16, n)
    scalar = _run_adamw(bf16, n, dict.fromkeys(_STREAMS, 1))
    _assert_states_equal(vec, scalar)
    # the update moved something, and the moments are non-zero from step 1 on
    master0, _ = _adam_inputs(bf16, n)
    assert not torch.equal(vec[0][1], master0)
    assert vec[0][2].abs().max() > 0 and vec[0][3].abs().max() > 0


@pytest.mark.parametrize("stream", _STREAMS)
def test_adamw_one_misaligned_pointer_takes_scalar_path(stream):
    n = 65537
    vec = _aligned_run(True, n)
    one = _run_adamw(True, n, dict(_ALIGNED, **{stream: 1}))
    _assert_states_equal(vec, one)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", _SIZES)
def test_l2norm_sq_aligned_and_misaligned(bf16, n):
    _, grads = _adam_inputs(bf16, n)
    ref = grads[0].double().pow(2).sum().item()
    for offset in (0, 1):
        x = _place(grads[0], offset)
        chunk = _ext().adamw_chunk_elems()
        desc = torch.tensor([[x.data_ptr() + s * x.element_size(), min(chunk, n - s)]
                             for s in range(0, n, chunk)], dtype=torch.int64, device="cuda")
        out = torch.zeros(1, dtype=torch.float32, device="cuda")
        _ext().l2norm_sq(desc, bf16, out)
        got = out.item()
        print(f"l2norm_sq n={n} offset={offset}: {got!r} vs fp64 {ref!r}")
        # 1e-5 relative, the bar of test_fused_adamw_matches_torch_on_gpu
        assert math.isfinite(got) and abs(got - ref) <= 1e-5 * ref
