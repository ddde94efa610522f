"""The two bf16 decode-GEMV anchors against the exact references of tests/_gemv_reference.py: usdm_gemv in all nine (rows per wave,
GLU, waves) instantiations and lm_head mode at the smallest shapes that reach them, and usdm_gemv_batch in its VALU form (2 ... 4
items) and in every matrix-core variant, tile height and mode.  Integer cases compare bit patterns in two launches (round_bf16 off:
the exact sum; on: its bf16 roundings, y16 = bf16(y32)); NaN fills every operand gap and the sentinel surrounds every output.

Measured on an MI355X: SwiGLU without round_bf16 reaches at most 0.23 of its bound (4 x torch's float32 error) and differs from the
fp64 reference with HF's rounding points on none of its outputs with round_bf16; of the RMSNorm probe's elements at most 1.04 % of a
case equal only the reference at rstd (1 + DELTA)."""
import ctypes

import pytest
import torch

from tests import _gemv_reference as R
from tests._gemv_reference import BF, F32, F64

pytestmark = pytest.mark.gpu

OUT_DTYPE = {"y32": F32, "y16": BF, "part_val": F32, "part_idx": torch.int32, "x_out": BF}
EXP_OF = {"y32": "y", "y16": "y", "part_val": "part_val", "part_idx": "part_idx", "x_out": "x_out"}


class Run:
    """a case on the device: its operands uploaded once, launches into fresh sentinel-filled outputs"""

    def __init__(self, c, dev, d=None, fmt=None):
        """d, fmt="bf16": the bf16 entry point on the logical weights of a quantized case that is already built (its twin)"""
        self.c, self.dev, self.d = c, dev, R.build(c) if d is None else d
        self.fmt = c.fmt if fmt is None else fmt
        up = lambda t: None if t is None else t.to(dev)
        d = self.d
        self.W, self.ldw = R.device_weight(c, d, dev, self.fmt)       # (a quantized format: quantized here, once per case, on the device)
        self.x, self.norm_w, self.res, self.ban, self.x_delta = up(d.x), up(d.norm_w), up(d.res), up(d.ban), up(d.x_delta)
        self.skip = torch.ones(1, dtype=torch.int32, device=dev) if c.skip else None
        self.ks = None
        if c.ks:
            self.ksf, self.nt16 = R.ks_floats(c.N, c.K), R.cdiv(c.N, 16)
            cnt = torch.cat([torch.zeros(self.nt16, dtype=torch.int32), R.sentinel((4,), torch.int32)]).to(dev)
            self.ks = (R.sentinel((self.ksf + 64,), F32, dev), cnt)
        self.mkw = {}
        if c.merge:             # the merged-attention input; hand-off form: K / 2 granules, 16 more that no launch may touch, the error word
            self.mkw["merge"] = (up(d.pm_buf), up(d.pl_buf), up(d.po_buf), c.NS)
            if c.merge == "cmb":
                self.gran, self.cmb_err = torch.empty(c.K // 2 + 16, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
                self.mkw["cmb"] = (self.gran, self.cmb_err)

    def sizes(self):
        c = self.c
        return {"y32": (c.B + 1) * c.y_bs, "y16": (c.B + 1) * c.y_bs, "part_val": (c.B + 1) * c.part_bs, "part_idx": (c.B + 1) * c.part_bs, "x_out": c.K + R.PAD}

    def launch(self, rbf, names, alt=False, inplace=False):
        """names: the outputs to pass -> {name: flat CPU tensor}; alt: over the second sentinel; inplace: y16 starts as the residual (its
        gaps hold the fill) and is passed as both"""
        from usdm_amd import ops
        c, dev = self.c, self.dev
        out = {n: (R.alt_sentinel if alt else R.sentinel)((self.sizes()[n],), OUT_DTYPE[n], dev) for n in names}
        res = self.res
        if inplace:
            view = out["y16"].view(c.B + 1, c.y_bs)
            view[:c.B, :c.nout] = self.d.rl.to(BF).to(dev)
            res = out["y16"]
        kw = dict(N=c.N, K=c.K, ldw=self.ldw, norm_w=self.norm_w, eps=R.EPS, act=c.act, round_bf16=rbf, residual=res, y16=out.get("y16"), y32=out.get("y32"),
                  ban=self.ban, part_val=out.get("part_val"), part_idx=out.get("part_idx"), idx_offset=c.idx_offset)
        if c.nb:
            bkw = dict(nb=c.nb, x_bs=c.x_bs, y_bs=c.y_bs, res_bs=c.res_bs, part_bs=c.part_bs, ks=self.ks, **kw)
            if c.fmt == "fp8" and c.mfma and self.fmt == "fp8":
                ops.gemv_fp8_mfma(self.W, self.x, form=c.form, **bkw)
            else:               # (the twin of an usdm_gemv_fp8_mfma case: form 1 is what its form 0 must equal)
                ops.gemv_batch(self.W, self.x, form=1 if (c.fmt == "fp8" and c.mfma and c.form == 0) else c.form, **bkw)
        else:
            if c.merge == "cmb":            # the tags are zero when the launch starts: the test clears them itself, every time
                self.gran[:c.K // 2], self.gran[c.K // 2:] = 0, R.GRAN_TAIL
                self.cmb_err.zero_()
            ops.gemv(self.W, self.x, x_delta=self.x_delta, x_out=out.get("x_out"), skip=self.skip, **self.mkw, **kw)
        torch.cuda.synchronize()
        if c.merge == "cmb":                # (self.granules: what the launch left in cmb_gran[K / 2])
            self.granules = self.gran[:c.K // 2].cpu()
            assert int(self.cmb_err.item()) == 0, f"{c.name}: cmb_err = {int(self.cmb_err.item())}"
            assert bool((self.gran[c.K // 2:].cpu() == R.GRAN_TAIL).all()), f"{c.name}: granules written past cmb_gran[K / 2]"
        if c.ks:
            part, cnt = self.ks[0].cpu(), self.ks[1].cpu()
            assert int(cnt[:self.nt16].abs().sum()) == 0, f"{c.name}: tile counters not back at zero"
            assert bool(R.is_sentinel(cnt[self.nt16:]).all()) and bool(R.is_sentinel(part[self.ksf:]).all()), f"{c.name}: written past the K-split scratch"
        return {n: t.cpu() for n, t in out.items()}

    def threads(self):
        from usdm_amd import _lib, ops
        c = self.c
        pv = torch.empty(1, device=self.dev) if c.lm_head else None
        W = self.W if self.fmt == "bf16" else self.W.q        # (the launch selection does not depend on the format: the bf16 arguments)
        a = ops.gemv(W, self.x, only_args=True, N=c.N, K=c.K, ldw=c.ldw, act=c.act, part_val=pv, part_idx=pv, **self.mkw)
        return _lib.lib.usdm_gemv_threads(ctypes.byref(a))


def _names(c, rbf):
    if c.fmt == "mxfp4":                                            # (usdm_gemv_mxfp4 has no y32 and no lm_head mode)
        return ["y16"]
    n = ["y32"] + (["y16"] if rbf and not c.lm_head else [])       # (lm_head mode has f32 logits only)
    if c.lm_head:
        n += ["part_val", "part_idx"]
    if c.delta:
        n.append("x_out")
    return n


def _exact(r, rbf, e, inplace=False):
    """one launch, every output bit for bit; owned elements that hold the sentinel's bits are read again over another fill"""
    c = r.c
    names = _names(c, rbf)
    got = r.launch(rbf, names, inplace=inplace)
    again = None
    for n in names:
        exp = e[EXP_OF[n]]
        R.check_exact(f"{c.name} rbf={int(rbf)} {n}", got[n], exp)
        amb = exp.owned & R.is_sentinel(got[n])
        if bool(amb.any()):
            again = r.launch(rbf, names, alt=True, inplace=inplace) if again is None else again
            assert torch.equal(R.bits(again[n])[amb], R.bits(got[n])[amb]), f"{c.name} {n}: owned elements never written"
    if "y16" in got and "y32" in got:
        own = e["y"].owned
        assert torch.equal(R.bits(got["y16"])[own], R.bits(got["y32"].to(BF))[own]), f"{c.name}: y16 is not y32 rounded to bf16"
    return got


def _twin(r):
    """a quantized case's logical weights are bf16 values that quantize losslessly (tests/test_gemv_exact_cpu.py), so the bf16 entry
    point on them must give the same bits; None for a bf16 case"""
    return None if r.fmt == "bf16" else Run(r.c, r.dev, d=r.d, fmt="bf16")


def _equals_twin(r, got, tw):
    for n in got:
        assert torch.equal(R.bits(got[n]), R.bits(tw[n])), f"{r.c.name} {n}: differs from the bf16 entry point on the same weights"


def _partials_follow_logits(c, got):
    """the partials hold the lowest-id arg-max of the logits the launch wrote"""
    lg = got["y32"].double().view(c.B + 1, c.y_bs)[:c.B, :c.N]
    val, idx = R.partials(c, lg)
    pv, pi = got["part_val"].view(c.B + 1, c.part_bs)[:c.B, :val.shape[1]], got["part_idx"].view(c.B + 1, c.part_bs)[:c.B, :val.shape[1]]
    assert torch.equal(R.bits(pv), R.bits(val.float())) and torch.equal(pi, idx.to(torch.int32)), f"{c.name}: partials do not follow the logits written"


def _swiglu(r):
    """round_bf16 off: within SWIGLU_TOL of fp64 silu(g) u; on: within one bf16 ulp of the reference with HF's rounding points, at most
    FLIP_CAP of the outputs differing at all"""
    c = r.c
    t = _twin(r)
    e = R.expected(c, r.d, rbf=False)["y"]
    if t is None:
        got = r.launch(False, ["y32"])["y32"]
    else:           # the bound on y32 (MXFP4 has none: on the twin's, whose y16 = bf16(y32) it must equal), and the twin's bits
        q, tw = r.launch(False, _names(c, True)), t.launch(False, ["y32", "y16"])
        got = q["y32"] if "y32" in q else tw["y32"]
        _equals_twin(r, q, tw)
        R.check_guard(f"{c.name} y16", q["y16"], e, R.bf16_ulp(e.vals))
        assert torch.equal(R.bits(tw["y16"])[e.owned], R.bits(tw["y32"].to(BF))[e.owned]), f"{c.name}: y16 is not y32 rounded to bf16"
    own = e.owned
    tol = R.SWIGLU_TOL * torch.where(own, torch.maximum(e.vals.abs(), e.up.abs()), torch.zeros((), dtype=F64))
    R.check_guard(f"{c.name} y32", got, e, tol)
    err = torch.where(own, (got.double() - e.vals).abs(), torch.zeros((), dtype=F64))
    ratio = float((err[own] / tol[own]).nan_to_num(0.0).max())
    print(f"[gemv] {c.name}: SwiGLU worst error / bound {ratio:.3f}")
    assert bool((err <= tol).all()), f"{c.name}: {ratio:.3f} x the SwiGLU bound"
    e = R.expected(c, r.d, rbf=True)["y"]
    got = r.launch(True, _names(c, True))
    if t is not None:
        _equals_twin(r, got, t.launch(True, list(got)))
    for n, g in got.items():
        R.check_guard(f"{c.name} {n}", g, e, R.bf16_ulp(e.vals))
        dd = (g.double() - e.vals).abs()[own]
        nd = int((dd != 0).sum())
        print(f"[gemv] {c.name} {n}: {nd} of {dd.numel()} differ with round_bf16")
        assert bool((dd <= R.bf16_ulp(e.vals[own])).all()) and nd <= R.FLIP_CAP * dd.numel(), (c.name, n)
    if "y32" in got:
        assert torch.equal(R.bits(got["y16"])[own], R.bits(got["y32"].to(BF))[own]), f"{c.name}: y16 is not y32 rounded to bf16"
    return ratio


def _probe(r):
    """every element equals the reference at rstd (1 - DELTA) or at rstd (1 + DELTA) -> the share that equals only the latter"""
    c = r.c
    lo, hi = (R.expected(c, r.d, rbf=not c.glu, scale=s) for s in (1 - R.DELTA, 1 + R.DELTA))
    own = lo["y"].owned
    t = _twin(r)
    if c.glu:       # y = silu(x') x': within the SwiGLU bound of either reference (a bf16 step of x' is 2^-8, the bound 7e-7)
        if t is None:
            got = r.launch(False, ["y32"])
        else:       # (MXFP4 has no y32: the bound on the twin's, whose y16 = bf16(y32) it must equal)
            q, got = r.launch(False, _names(c, True)), t.launch(False, ["y32", "y16"])
            _equals_twin(r, q, got)
            R.check_guard(f"{c.name} y16", q["y16"], lo["y"], 1e-5)
            assert torch.equal(R.bits(got["y16"])[own], R.bits(got["y32"].to(BF))[own]), f"{c.name}: y16 is not y32 rounded to bf16"
        g = got["y32"].double()
        R.check_guard(f"{c.name} y32", got["y32"], lo["y"], 1e-5)
        ok = [(g - e["y"].vals).abs() <= R.SWIGLU_TOL * torch.maximum(e["y"].vals.abs(), e["y"].up.abs()) for e in (lo, hi)]
    else:           # round_bf16 rounds bf16 values: y32 = y16 = x'[k_n]
        got = r.launch(True, _names(c, True))
        if t is not None:
            _equals_twin(r, got, t.launch(True, list(got)))
        main = "y32" if "y32" in got else "y16"
        R.check_guard(f"{c.name} {main}", got[main], lo["y"], 0.0)
        if "y16" in got and main == "y32":
            R.check_guard(f"{c.name} y16", got["y16"], lo["y"], 0.0)
            assert torch.equal(R.bits(got["y16"])[own], R.bits(got["y32"].to(BF))[own]), f"{c.name}: y16 is not y32 rounded to bf16"
        ok = [R.bits(got[main]) == R.bits(e["y"].vals.to(got[main].dtype)) for e in (lo, hi)]
        if c.lm_head:
            _partials_follow_logits(c, got)
            for n in ("part_val", "part_idx"):
                R.check_guard(f"{c.name} {n}", got[n], lo[n], INF_TOL)
    bad = own & ~ok[0] & ~ok[1]
    assert not bool(bad.any()), f"{c.name}: {int(bad.sum())} of {int(own.sum())} elements equal neither reference, first at {int(bad.nonzero()[0]) if bool(bad.any()) else -1}"
    share = float((own & ok[1] & ~ok[0]).sum()) / int(own.sum())
    print(f"[gemv] {c.name}: {100 * share:.2f} % of the elements equal only the reference at rstd (1 + DELTA)")
    return share


INF_TOL = float("inf")      # check_guard on the partials of a probe: only that nothing outside the owned ones is written


def run_case(c, dev, r=None):
    r = Run(c, dev) if r is None else r
    if not c.nb:
        assert r.threads() == c.threads(), f"{c.name}: usdm_gemv_threads says {r.threads()}, the mirror {c.threads()}"
    if c.skip:
        for rbf in (False, True):
            for n, g in r.launch(rbf, _names(c, True)).items():
                assert bool(R.is_sentinel(g).all()), f"{c.name}: {n} written although *skip = 1"
        return
    if c.kind == "probe":
        return _probe(r)
    if c.kind == "swiglu":
        return _swiglu(r)
    x0 = R.bits(r.x)
    e0 = R.expected(c, r.d, rbf=False)                  # (lm_head mode: the logits are bf16 whatever round_bf16 says, the same reference)
    got0 = _exact(r, False, e0)
    if c.lm_head:
        _partials_follow_logits(c, got0)
    e = R.expected(c, r.d, rbf=True)
    got = _exact(r, True, e, inplace=c.inplace)
    if c.lm_head:
        _partials_follow_logits(c, got)
    if c.ks:                        # the same scratch again: identical bits whichever workgroup arrives last
        again = r.launch(True, _names(c, True), inplace=c.inplace)
        assert all(torch.equal(R.bits(again[n]), R.bits(got[n])) for n in got), f"{c.name}: the K-split sum depends on the arrival order"
    assert torch.equal(R.bits(r.x), x0), f"{c.name}: x changed"


def _run_all(cases, dev, what, run=run_case):
    worst = [v for v in (run(c, dev) for c in cases) if v is not None]
    if worst:
        print(f"[gemv] {what}: worst {max(worst):.4f}")


INSTS = list(R.VALU_INST) + ["lm"]


@pytest.mark.parametrize("inst", INSTS, ids=R.inst_id)
def test_gemv_plain(dev, inst):
    """usdm_gemv, integer operands over the instantiation's K ladder (below, at and above one iteration, the ring depth and the
    workgroup's first pass over x; K = 16384 on the small shapes): plain with a residual, SwiGLU on the GLU instantiations, logits
    and partials in lm_head mode"""
    _run_all(R.valu_plain_cases(inst), dev, "SwiGLU error / bound")


@pytest.mark.parametrize("inst", INSTS, ids=R.inst_id)
def test_gemv_norm_exact(dev, inst):
    """fused RMSNorm on x = +-2: x' = +-norm_w exactly, so the projection after the norm is an integer case"""
    _run_all(R.valu_norm_exact_cases(inst), dev, "SwiGLU error / bound")


@pytest.mark.parametrize("inst", INSTS, ids=R.inst_id)
def test_gemv_norm_probe(dev, inst):
    """fused RMSNorm read back through unit-vector rows at K = 504 and 8 x threads + 8: every x' equals the fp64 reference at
    rstd (1 -+ 2^-17)"""
    _run_all(R.valu_probe_cases(inst), dev, "share of the (1 + DELTA) reference")


def test_gemv_lm_head_bans(dev):
    """no ban array, a banned workgroup, a banned wave in a live workgroup, scattered bans, the last row; idx_offset != 0; both settings of
    round_bf16 (the logits are bf16 either way)"""
    _run_all(R.lm_head_cases(), dev, "")


@pytest.mark.parametrize("inst", R.DELTA_INST, ids=R.inst_id)
def test_gemv_x_delta(dev, inst):
    """x' = bf16(x + bf16(x_delta)) feeds the projection (and the RMSNorm) and lands in x_out; x itself is unchanged"""
    _run_all(R.delta_cases(inst), dev, "")


@pytest.mark.parametrize("inst", R.DELTA_INST, ids=R.inst_id)
def test_gemv_skip(dev, inst):
    """*skip = 1: no output is touched"""
    _run_all(R.skip_cases(inst), dev, "")


@pytest.mark.parametrize("inst", R.BATCH_INST + ("lm",), ids=R.inst_id)
@pytest.mark.parametrize("nb", R.VALU_NB)
def test_gemv_batch_valu(dev, nb, inst):
    """usdm_gemv_batch form -1: every item against its own reference (different data per item, strided with NaN between)"""
    _run_all(R.valu_plain_cases(inst, nb) + R.valu_norm_exact_cases(inst, nb), dev, "SwiGLU error / bound")
    _run_all(R.valu_probe_cases(inst, nb), dev, "share of the (1 + DELTA) reference")


@pytest.mark.parametrize("nb", R.VALU_NB)
def test_gemv_batch_valu_lm_head_bans(dev, nb):
    _run_all(R.lm_head_cases(nb), dev, "")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_batch_matrix_cores(dev, nb):
    """N = 37 over every variant: held and streamed activations, both load patterns at K = 4096 and 14336, K split in 3, 7 and 8
    slices (counters back at zero, the same bits on the same scratch); plain + residual, in place in the round_bf16 launch"""
    _run_all(R.mfma_ladder_cases(nb), dev, "")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_batch_matrix_cores_tile_rows(dev, nb):
    """12-row tiles (N = 6144) and ragged 16-row tiles (N = 4085); N = 37 above runs 8-row tiles"""
    _run_all(R.mfma_tile_cases(nb), dev, "")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_batch_matrix_cores_swiglu(dev, nb):
    _run_all(R.mfma_swiglu_cases(nb), dev, "SwiGLU error / bound")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_batch_matrix_cores_norm(dev, nb):
    """both RMSNorm families on the held activations (K <= 4096); the probe covers all of K at K = 4096"""
    cases = R.mfma_norm_cases(nb)
    _run_all([c for c in cases if c.kind != "probe"], dev, "SwiGLU error / bound")
    _run_all([c for c in cases if c.kind == "probe"], dev, "share of the (1 + DELTA) reference")


@pytest.mark.parametrize("nb", R.MFMA_NB)
def test_gemv_batch_matrix_cores_lm_head(dev, nb):
    """N = 1003 with all five ban patterns (no ban array among them): one partial per workgroup, the rest of part_bs reads "no candidate" """
    _run_all(R.lm_head_cases(nb, mfma=True), dev, "")


def test_gemv_batch_matrix_cores_refuse_a_partial_swiglu_block(dev):
    """SwiGLU rows come in blocks of 16 gate + 16 up rows: N = 80 would put the last up rows past W, and is refused before any launch"""
    from usdm_amd import _lib, ops
    W, x, y = torch.zeros(96, 256, dtype=BF, device=dev), torch.zeros(5, 256, dtype=BF, device=dev), torch.zeros(5, 48, device=dev)
    with pytest.raises(_lib.UsdmError, match="swiglu needs N"):
        ops.gemv_batch(W, x, nb=5, x_bs=256, y_bs=48, form=1, N=80, K=256, act=R.ACT_SWIGLU, y32=y)
