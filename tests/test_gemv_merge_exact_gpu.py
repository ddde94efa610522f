"""usdm_gemv with the merged-attention input against the exact references of tests/_gemv_reference.py: GEMV_MRG on (1 row per wave,
16 waves) and on (1, 4 waves), and the hand-off form GEMV_CMB on (1, 16 waves), the o_proj of the shipped decode step.  With a real
weight matrix (ldw = K + 8, NaN gaps), residuals, both round_bf16 settings, ragged last workgroups and every K / NS at which the two
x-staging prologues take another path.  Family "exact": the merge gives the integer x of the integer cases in any summation order,
so every output is compared bit for bit; family "probe": real softmax weights read back through unit-vector rows, every element a
bf16 value within half a bf16 ulp + B of the fp64 merge (B: module docstring of the reference).

Measured on an MI355X: the worst (|got - ref64| - half ulp) / B of a probe case is 0.0003 (mrg16 at NS = 64 and cmb at NS = 21, one
element each that is not bf16(ref64); every other case stays inside half an ulp alone), so the derived bound is never near.  The
slowest id is test_gemv_merge_exact[cmb-N4096-K4224] at 1.0 s; the file takes 7 s.

Two breaks of llm_k.hip were tried locally (never committed), each against this file and tests/test_llm_gpu.py:
  * MRG prologue, every clamped load past NS weighted 1 instead of 0: eleven ids here fail (all nine MRG shapes, both MRG probes) -
    and so do test_llm_gpu.py::test_attn_decode[5, 130, 700], whose NS = 3 launch adds five whole splits, far outside its 2e-2.
    Narrowed to the clamped loads of the chunks after the first (NS = 9 ... 15, 17 ...; the older tests run NS = 3 and 8, one
    chunk): the same eleven ids fail here, at NS = 9 (all outputs near 1e31: the 2^100 of a dead split), test_llm_gpu.py passes.
  * CMB gather, zero staged for granules from 2048 on: test_gemv_merge_exact[cmb-N4096-K4224] and [cmb-N4096-K8192] fail here,
    test_llm_gpu.py (K = 4096) passes."""
import pytest
import torch

from tests import _gemv_reference as R
from tests._gemv_reference import BF
from tests.test_gemv_exact_gpu import Run, _run_all, run_case       # (run_case: the two _exact launches of an integer case)

pytestmark = pytest.mark.gpu

SHAPES = [(f, s) for f in R.MERGE_FORMS for s in R.MERGE_SHAPES[f]]


def _granules_hold(r, x, what):
    """every granule of cmb_gran[K / 2] has tag 1 and holds the bf16 pair of x (fp64 [K], bf16 values)"""
    g, want = r.granules, R.granules(x)
    assert bool(((g >> 32) == 1).all()), f"{r.c.name}: {int(((g >> 32) != 1).sum())} granules without tag 1 {what}"
    bad = g != want
    assert not bool(bad.any()), f"{r.c.name}: {int(bad.sum())} granules differ from the merged x {what}, first at {int(bad.nonzero()[0]) if bool(bad.any()) else -1}"


def _merge_exact(c, dev):
    """the two launches of run_case (round_bf16 off and on, in place where the case says so: every output bit for bit, y16 = bf16(y32),
    the x buffer unchanged), then y32 alone and y16 alone; hand-off form: the granules after every launch, and the same bits again
    on re-zeroed tags"""
    r = Run(c, dev)
    x = R.x_prime(c, r.d)[0][0]
    run_case(c, dev, r)
    if c.merge == "cmb":
        _granules_hold(r, x, "after the round_bf16 launch")
    e = R.expected(c, r.d, rbf=True)["y"]
    first = None
    for names in (["y32"], ["y16"], ["y32", "y16"]):
        got = r.launch(True, names)
        for n in names:
            R.check_exact(f"{c.name} {'+'.join(names)}: {n}", got[n], e)
        if c.merge == "cmb":
            _granules_hold(r, x, f"with {'+'.join(names)}")
            first = r.granules if first is None else first
            assert torch.equal(first, r.granules), f"{c.name}: another launch left other granules"


def _merge_skip(c, dev):
    """*skip = 1 (run_case: no output element is touched in either launch; Run.launch: cmb_err stays 0 and nothing is written past
    cmb_gran[K / 2]).  The header promises nothing about the K / 2 granules of a skipped launch: nothing is asserted about them"""
    assert c.skip
    run_case(c, dev)


def _merge_probe(c, dev):
    """round_bf16 off, y32[n] = x[k_n]: a bf16 value within half a bf16 ulp of the fp64 merge + B, every element -> the worst
    (|got - ref64| - half ulp) / B"""
    r = Run(c, dev)
    assert r.threads() == c.threads()
    ref, B = (t[r.d.kpos] for t in R.merge_ref(c, r.d))
    e = R.expected(c, r.d, rbf=False)["y"]
    got = r.launch(False, ["y32"])["y32"]
    R.check_guard(f"{c.name} y32", got, e, float("inf"))
    own = e.owned
    assert int(own.sum()) == c.N == ref.numel() and bool(own[:c.N].all())
    g = got[:c.N]
    assert torch.equal(R.bits(g), R.bits(g.to(BF).float())), f"{c.name}: y32 holds values that are not bf16"
    excess = ((g.double() - ref).abs() - R.bf16_ulp(ref) / 2) / B
    ratio = float(excess.max())
    print(f"[gemv] {c.name}: worst (|got - ref64| - half ulp) / B = {ratio:.4f}; {int((R.rbf64(ref) != g.double()).sum())} of {c.N} elements are not bf16(ref64)")
    bad = ~(excess <= 1.0)
    assert not bool(bad.any()), f"{c.name}: {int(bad.sum())} of {c.N} elements outside half a bf16 ulp + B, worst {ratio:.3f} B, first at row {int(bad.nonzero()[0]) if bool(bad.any()) else -1}"
    if c.merge == "cmb":        # the granules hold what the rows read back: tag 1 and the bits of y32
        gr = r.granules
        assert bool(((gr >> 32) == 1).all()), f"{c.name}: granules without tag 1"
        k = r.d.kpos
        xb = torch.where(k % 2 == 0, gr[k // 2] & 0xffff, (gr[k // 2] >> 16) & 0xffff)
        assert torch.equal(xb, R.bits(g.to(BF)).to(torch.int64) & 0xffff), f"{c.name}: the granules differ from the x the projection used"
    return ratio


@pytest.mark.parametrize("form,shape", SHAPES, ids=[f"{f}-N{s[0]}-K{s[1]}" for f, s in SHAPES])
def test_gemv_merge_exact(dev, form, shape):
    """the exact family at one (N, K): NS either side of a chunk of 8 (MRG) / a group of four (CMB), the whole NS ladder at one shape per
    instantiation; plain, with a residual, with the residual in place in the round_bf16 launch"""
    _run_all(R.merge_exact_cases(form, shape), dev, "", run=_merge_exact)


@pytest.mark.parametrize("form", R.MERGE_FORMS)
def test_gemv_merge_skip(dev, form):
    _run_all(R.merge_skip_cases(form), dev, "", run=_merge_skip)


@pytest.mark.parametrize("form", R.MERGE_FORMS)
def test_gemv_merge_probe(dev, form):
    """real softmax weights: NS = 9 and 64 (MRG), 5, 21 and 64 (CMB), at K = 4096 (all of K is read) and at K = 1152 with 37 rows"""
    _run_all(R.merge_probe_cases(form), dev, "worst (|got - ref64| - half ulp) / B", run=_merge_probe)
