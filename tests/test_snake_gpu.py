"""GPU: usdm_aa_snake (aa_snake_kernel of usdm_amd/csrc/bigvgan_k.hip, the fused Activation1d(SnakeBeta) of BigVGAN) called
directly through usdm_amd.ops.aa_snake and pinned by the check families of tests/_snake_reference.py, which tests/test_snake_cpu.py
shows to be right and to reject ten planted defects of a float32 emulation of the kernel:

  1 test_exact_*     alpha = 0: an integer-exact FIR with asymmetric integer taps; out32 == int64 reference, out16 == its bf16
  2 test_one_tap     one-tap filters: every output is one snake evaluation of one known sample (or a replicated end, or 0), against
                     float64 under the derived bound tol() of _snake_reference
  3 test_chunking    real taps: L and the choice of outputs change no bit; out16 = bf16(out32)
  4 test_strides     ldx, ldo, an offset view: the bits of the dense call
  5 test_refusals    what the launcher must refuse, with nothing written

Every launch reads x from a buffer with a row of NaN before and after it, NaN in the stride gaps and NaN in the padding channels
[Creal, C) (alpha and beta hold NaN there too), and writes into buffers pre-filled with a NaN of a known payload, which must
survive bit for bit everywhere outside the T x C block (_Run.__call__ asserts it on every launch of every family).

Measured on an MI355X, worst |out32 - ref| / tol of family 2: 0.495 (per setting in test_one_tap's docstring).
"""
import numpy as np
import pytest
import torch

from tests import _snake_reference as R

pytestmark = pytest.mark.gpu
SENT32 = 0x7fc00bad          # quiet NaNs with a payload: the kernel's own NaN, had it one, would not carry it
SENT16 = 0x7fcb


class _Run:
    """the `run` of the check_* functions on the device: (case, L, outs, ldx, ldo, xoff) -> (out32 [T][C] float32 or None,
    out16 [T][C] bf16 bits or None), after asserting that nothing outside that block was written"""

    def __init__(self, dev):
        self.dev = dev
        self.params = {}

    def _param(self, a):
        if id(a) not in self.params:
            self.params[id(a)] = (a, torch.from_numpy(a).to(self.dev))          # (a is kept: its id stays its own)
        return self.params[id(a)][1]

    def buffers(self, T, ldo):
        o32 = torch.full(((T + 2) * ldo,), SENT32, dtype=torch.int32, device=self.dev).view(torch.float32)
        o16 = torch.full(((T + 2) * ldo,), SENT16, dtype=torch.int16, device=self.dev).view(torch.bfloat16)
        return o32, o16

    @staticmethod
    def untouched(buf, T, C, ldo, what, written=True):
        """-> the [T][C] block of an output buffer as integers, after checking the sentinel everywhere else (everywhere, if not written)"""
        bits = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16).cpu().numpy().reshape(T + 2, ldo)
        sent = SENT32 if buf.dtype == torch.float32 else SENT16
        outside = np.ones(bits.shape, bool)
        if written:
            outside[1:T + 1, :C] = False
        bad = outside & (bits != sent)
        assert not bad.any(), f"{what}: written outside its [{T}][{C}] block at (row, column) {np.argwhere(bad)[:4].tolist()} of [{T + 2}][{ldo}]"
        return np.ascontiguousarray(bits[1:T + 1, :C])

    def __call__(self, case, L=None, outs="both", ldx=None, ldo=None, xoff=0):
        from usdm_amd import ops
        T, C = case["x"].shape
        ldx, ldo = ldx or case.get("ldx", C), ldo or case.get("ldo", C)
        buf, start = R.strided_input(case["x"], ldx, xoff)
        xd = torch.from_numpy(buf).to(self.dev)
        o32, o16 = self.buffers(T, ldo)
        ops.aa_snake(xd[start:], self._param(case["alpha"]), self._param(case["beta"]), case["fup"], case["fdn"], T=T, C=C,
                     Creal=case["Creal"], logscale=bool(case["logscale"]), L=case["L"] if L is None else L, ldx=ldx, ldo=ldo,
                     out32=o32[ldo:] if outs != "out16" else None, out16=o16[ldo:] if outs != "out32" else None)
        torch.cuda.synchronize()
        what = f"{case['name']} (L={L}, {outs}, ldx={ldx}, ldo={ldo}, xoff={xoff})"
        g32 = self.untouched(o32, T, C, ldo, what + " out32", outs != "out16")
        g16 = self.untouched(o16, T, C, ldo, what + " out16", outs != "out32")
        return (g32.view(np.float32) if outs != "out16" else None), (g16.view(np.uint16) if outs != "out32" else None)


@pytest.fixture(scope="module")
def run(dev):
    return _Run(dev)


# ------------------------------------------------------------------------------------------------------------------ family 1
@pytest.mark.parametrize("T", R.T_LIST)
def test_exact_chunks(run, T):
    """alpha = 0, beta = 1, logscale = 0, x integers of [-3, 3], asymmetric integer taps, C = 34 with 33 real channels, every L of
    {0, 1, 2, 3, 8, 16, 32}: chunk seams at every distance from the ends (for T < 6 the two pads share a window).  Every partial sum
    is an integer below 2^24, so out32 == the int64 reference and out16 == its bf16 rounding; channel 33 is 0 although its x, alpha
    and beta are NaN."""
    for c in R.exact_cases(T):
        R.check_exact(c, run)


@pytest.mark.parametrize("T", R.EXACT_SHAPE_T)
def test_exact_shapes(run, T):
    """the same at C in {2, 32, 34, 66} (one pair; a full column block; blocks with one and with 17 idle pairs) x Creal in
    {C, C - 1, 1} x (ldx, ldo) in {(C, C), (C + 2, C + 6)}"""
    for c in R.exact_shape_cases(T):
        R.check_exact(c, run)


# ------------------------------------------------------------------------------------------------------------------ family 2
@pytest.mark.parametrize("setting", R.ONE_TAP_SETTINGS)
def test_one_tap(run, setting):
    """fup = one 0.5 at index 5 or 6, fdn = one 1.0 at j0 = 0..11: out32[t] is v~[2t - 5 + j0], one snake evaluation (or exactly 0 on
    the empty phase), against float64 under tol() (derived in _snake_reference's docstring from 4 / 3 / 2.5 ulp for sin / exp /
    reciprocal and 0.5 ulp per float32 operation); out16 = bf16(out32) bit for bit.  Per-channel alpha and beta, all different, the
    two of a pair far apart.  Settings: logscale (+ T = 1, 2, 3 with every filter pair); snake (alpha and beta one tensor); beta0
    (beta = 0 without logscale: 1 / 1e-9, finite); |x a| around 1e-3, around 1 and up to 1e4 without logscale (the sine's argument
    is then the float32 product in the reference too).

    Measured on an MI355X (first run, tol as derived before it), worst |out32 - ref| / tol: logscale 0.462, snake 0.451, beta0 0.188,
    arg1e-3 0.495, arg1 0.428, arg1e4 0.476 (the float32 emulation on the CPU: 0.495 over all).  Just under a half is what the
    final add alone gives where the sin^2 term is small: its rounding is half an ulp of a bound of one (the add's and the
    output's half ulp)."""
    worst = 0.0
    for c in R.one_tap_cases(setting):
        worst = max(worst, R.check_one_tap(c, run))
    print(f"[snake] family 2 {setting}: worst |out32 - ref| / tol = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ family 3
@pytest.mark.parametrize("T", R.T_LIST)
def test_chunking(run, T):
    """the production taps, x of std 1.5, logscale parameters of std 0.4, C = 34 / Creal = 33: out32 and out16 at every L are the
    bits of L = 0, as are out32 alone and out16 alone (at L = 0 and 3); out16 is the bf16 rounding of out32"""
    R.check_chunking(R.chunking_case(T), run)


# ------------------------------------------------------------------------------------------------------------------ family 4
@pytest.mark.parametrize("T,C", R.STRIDE_SHAPES)
def test_strides(run, T, C):
    """ldx and ldo in {C, C + 2, C + 6} and x starting two floats into its buffer: the bits of the dense call (the gaps hold NaN on
    the way in and keep their sentinel on the way out)"""
    R.check_strides(R.stride_case(T, C), run)


# ------------------------------------------------------------------------------------------------------------------ family 5
def test_refusals(run, dev):
    """odd C, odd ldx / ldo, Creal > C, T = 0, no output, null x / alpha / beta, x or out32 off an 8-byte boundary, out16 off a 4-byte
    one: an error, and not one element of either output buffer written"""
    from usdm_amd import _lib, ops
    case = R.stride_case(5, 34)
    T, C = case["x"].shape
    ld = C + 2                                             # (room for the odd strides and the shifted pointers)
    buf, start = R.strided_input(case["x"], ld, 2)
    xd = torch.from_numpy(buf).to(dev)
    al, be = run._param(case["alpha"]), run._param(case["beta"])

    def refused(what, **kw):
        o32, o16 = run.buffers(T, ld)
        a = dict(x=xd[start:], alpha=al, beta=be, T=T, C=C, Creal=case["Creal"], ldx=ld, ldo=ld, out32=o32[ld:], out16=o16[ld:])
        a.update({k: (v(a[k]) if callable(v) else v) for k, v in kw.items()})
        x, alpha, beta = (a.pop(k) for k in ("x", "alpha", "beta"))
        with pytest.raises(_lib.UsdmError, match=what):
            ops.aa_snake(x, alpha, beta, case["fup"], case["fdn"], **a)
        torch.cuda.synchronize()
        run.untouched(o32, T, C, ld, f"refused ({kw}) out32", written=False)
        run.untouched(o16, T, C, ld, f"refused ({kw}) out16", written=False)

    refused("bad T/C", C=33)
    refused("bad T/C", Creal=35)
    refused("bad T/C", T=0)
    refused("strides", ldx=ld + 1)
    refused("strides", ldo=ld - 1)
    refused("no output", out32=None, out16=None)
    refused("null", x=None)
    refused("null", alpha=None)
    refused("null", beta=None)
    refused("aligned", x=lambda t: t[1:])
    refused("aligned", out32=lambda t: t[1:])
    refused("aligned", out16=lambda t: t[1:])
    refused("aligned", out32=None, out16=lambda t: t[1:])
    # and the same arguments, untouched, are accepted
    o32, o16 = run.buffers(T, ld)
    ops.aa_snake(xd[start:], al, be, case["fup"], case["fdn"], T=T, C=C, Creal=case["Creal"], ldx=ld, ldo=ld, out32=o32[ld:], out16=o16[ld:])
    torch.cuda.synchronize()
    got = run.untouched(o32, T, C, ld, "accepted out32").view(np.float32)
    ref, _ = run(case)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
