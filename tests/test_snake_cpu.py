"""CPU: the references of tests/_snake_reference.py are right (against torch's conv_transpose1d / conv1d with asymmetric taps and
against the oracle's Activation1d with the real ones), the float32 emulation of usdm_aa_snake passes every check family that
tests/test_snake_gpu.py runs on the device, every planted defect of the emulation is rejected by at least one family, and the
launcher refuses what the kernel cannot handle."""
import ctypes as C_

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import _snake_reference as R

F64 = torch.float64
ASYM_T = (1, 2, 3, 4, 5, 6, 7, 8, 9, 33)


def _torch_linear(x, fup, fdn):
    """Activation1d with the identity as its activation, from torch's own convolutions in float64: x [T][C] -> [T][C]"""
    C = x.shape[1]
    y = torch.from_numpy(x.T.copy()).to(F64)[None]
    wu = torch.tensor(fup, dtype=F64).view(1, 1, 12).expand(C, -1, -1)
    wd = torch.tensor(fdn, dtype=F64).view(1, 1, 12).expand(C, -1, -1)
    y = Fn.pad(y, (5, 5), mode="replicate")
    y = 2 * Fn.conv_transpose1d(y, wu, stride=2, groups=C)[..., 15:-15]
    y = Fn.pad(y, (5, 6), mode="replicate")
    return Fn.conv1d(y, wd, stride=2, groups=C)[0].T.numpy()


@pytest.mark.parametrize("T", ASYM_T)
def test_ref_linear_is_torchs_transposed_and_strided_convolution(T):
    """asymmetric integer taps: the orientation of fup and fdn and the two replicate pads, where the real taps cannot tell"""
    x = np.random.default_rng(T).integers(-3, 4, size=(T, 4))
    ref = R.ref_linear(x, np.array(R.FUP_INT), np.array(R.FDN_INT))
    assert ref.dtype == np.int64
    assert np.array_equal(ref.astype(np.float64), _torch_linear(x.astype(np.float64), R.FUP_INT, R.FDN_INT))
    assert np.array_equal(R.ref_linear(x.astype(np.float64), R.FUP_INT, R.FDN_INT), ref.astype(np.float64))
    if T > 1:
        for fu, fd in ((R.FUP_INT[::-1], R.FDN_INT), (R.FUP_INT, R.FDN_INT[::-1])):
            assert not np.array_equal(R.ref_linear(x, np.array(fu), np.array(fd)), ref), "the taps do not tell the orientation"
    # the snake reference with alpha = 0 is the same thing
    s = R.ref_snake(x, np.zeros(4), np.ones(4), R.FUP_INT, R.FDN_INT, 0, 4)
    assert np.array_equal(s, ref.astype(np.float64))


@pytest.mark.parametrize("T", ASYM_T)
@pytest.mark.parametrize("logscale", [0, 1])
def test_ref_snake_is_torchs_composition_with_asymmetric_taps(T, logscale):
    from oracle import bigvgan_oracle as BO
    rng = np.random.default_rng(50 + T)
    C = 4
    x, al, be = (rng.standard_normal(s).astype(np.float32) for s in ((T, C), C, C))
    fup, fdn = (rng.standard_normal(12).astype(np.float32) for _ in range(2))
    xt = torch.from_numpy(x.T.copy()).to(F64)[None]
    wu = torch.from_numpy(fup).to(F64).view(1, 1, 12).expand(C, -1, -1)
    wd = torch.from_numpy(fdn).to(F64).view(1, 1, 12).expand(C, -1, -1)
    y = 2 * Fn.conv_transpose1d(Fn.pad(xt, (5, 5), mode="replicate"), wu, stride=2, groups=C)[..., 15:-15]
    y = BO.snakebeta(y, torch.from_numpy(al).to(F64), torch.from_numpy(be).to(F64), bool(logscale))
    want = Fn.conv1d(Fn.pad(y, (5, 6), mode="replicate"), wd, stride=2, groups=C)[0].T.numpy()
    got = R.ref_snake(x, al, be, fup, fdn, logscale, C)
    # (without logscale the reference rounds u to float32 before the product with a: 2^-24 relative in the argument; the
    #  float32 1e-9f differs from 1e-9 by 3e-8 relative of a term that is itself 1e-9 of b)
    assert np.abs(got - want).max() <= (1e-12 if logscale else 2e-6) * np.abs(want).max()


@pytest.mark.parametrize("T", (1, 2, 7, 33))
def test_ref_snake_is_the_oracles_activation1d_with_the_real_taps(T):
    from oracle import bigvgan_oracle as BO
    c = R._real_case(T, 6, 5, 9 + T)
    taps = torch.from_numpy(c["fup"]).to(F64)
    assert torch.equal(taps, taps.flip(0)), "the production taps are symmetric"
    live = slice(0, c["Creal"])
    want = BO.activation1d(torch.from_numpy(c["x"][:, live].T.copy()).to(F64)[None], torch.from_numpy(c["alpha"][live]).to(F64),
                           torch.from_numpy(c["beta"][live]).to(F64), taps)[0].T.numpy()
    got = R.ref_snake(*(c[k] for k in ("x", "alpha", "beta", "fup", "fdn", "logscale", "Creal")))
    assert np.abs(got[:, live] - want).max() <= 1e-12 * np.abs(want).max()
    assert not got[:, c["Creal"]:].any()


def test_bf16_rounding_is_torchs():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 100
    x[:4] = torch.tensor([1.00390625, 1.01171875, -0.0, 21060.0])      # two exact ties (to even: down, up)
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x.numpy()), want)
    assert np.array_equal(R.bf16_value(want), x.to(torch.bfloat16).float().numpy())


def test_launcher_L_and_case_tables():
    assert [R.launcher_L(T, 34, 0) for T in (1, 257)] == [8, 8] and R.launcher_L(5, 34, 3) == 3
    assert R.launcher_L(500000, 1536, 0) == 32
    fam = R.families()
    seen = {(c["x"].shape[0], c["L"]) for c in fam["1 exact"][1]}
    assert seen >= {(T, L) for T in R.T_LIST for L in R.L_LIST}
    seen = {(c["x"].shape[0], c["L"]) for c in fam["2 one tap"][1]}
    assert seen >= {(T, L) for T in R.T_LIST for L in R.L_LIST}
    assert {(c["x"].shape[1], c["Creal"]) for c in fam["1 exact"][1]} >= {(C, r) for C in R.C_LIST for r in (C, C - 1, 1)}
    for name, (_, cases) in fam.items():
        for c in cases:
            assert np.isnan(c["x"][:, c["Creal"]:]).all() and np.isfinite(c["x"][:, :c["Creal"]]).all(), name
            assert np.isnan(c["alpha"][c["Creal"]:]).all() and np.isnan(c["beta"][c["Creal"]:]).all(), name
    snake = [c for c in fam["2 one tap"][1] if "snake" in c["name"]]
    assert snake and all(c["beta"] is c["alpha"] for c in snake)
    big = max(float(np.nanmax(np.abs(c["x"] * c["alpha"]))) for c in fam["2 one tap"][1] if "arg1e4" in c["name"])
    assert 9e3 < big <= 1e4


def test_emulation_passes_every_family():
    """the defect-free float32 emulation passes all that the device has to pass; prints its worst |got - ref| / tol of family 2"""
    run = R.emulated_run()
    for name, (check, cases) in R.families().items():
        worst = max((check(c, run) or 0.0) for c in cases)
        print(f"[snake] emulation, family {name}: {len(cases)} cases pass" + (f", worst |got - ref| / tol = {worst:.3f}" if worst else ""))
        assert name != "2 one tap" or 0 < worst <= 1.0


def _probe(cases, n):
    """about n cases, evenly spread (the whole sweep, ten times over, is minutes of emulation)"""
    return cases[::max(1, len(cases) // n)]


def test_every_planted_defect_is_rejected():
    fam = R.families()
    probes = {name: _probe(cases, 12 if name[0] in "12" else 3) for name, (_, cases) in fam.items()}
    table = {}
    for defect in R.DEFECTS:
        run = R.emulated_run(defect)
        for name, (check, _) in fam.items():
            hits = 0
            for c in probes[name]:
                try:
                    check(c, run)
                except AssertionError:
                    hits += 1
            if hits:
                table.setdefault(defect, {})[name] = hits
    print("[snake] defect -> the families that reject it (rejecting cases / cases tried)")
    for defect in R.DEFECTS:
        print(f"[snake]   {defect:18s} " + "; ".join(f"{k}: {v}/{len(probes[k])}" for k, v in table.get(defect, {}).items()))
    missed = [d for d in R.DEFECTS if d not in table]
    assert not missed, f"no family rejects {missed}"
    # the sharp families, not a tolerance, carry the structural defects
    for d in ("fdn_reversed", "fup_reversed", "phase_swapped", "v_zero_pad", "x_zero_pad", "pad_not_zeroed", "short_window"):
        assert "1 exact" in table[d], d
    for d in ("neighbour_params", "eps_omitted", "logscale_ignored"):
        assert "2 one tap" in table[d], d
    assert "3 chunking" in table["short_window"]


@pytest.mark.parametrize("setting", R.ONE_TAP_SETTINGS)
def test_a_neighbours_parameters_show_between_two_real_channels(setting):
    """with no padding channel (no NaN to give it away) every parameter setting of family 2 rejects alpha / beta of c ^ 1: the
    values of a pair are far enough apart for the bound"""
    c = R._one_tap_case(setting, 0, 5, 33, 0, C=R.C_MAIN, Creal=R.C_MAIN)
    assert R.check_one_tap(c, R.emulated_run()) <= 1.0
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_one_tap(c, R.emulated_run("neighbour_params"))


# ------------------------------------------------------------------------------------------------------------------ host refusals
PTR = 0x10000


def _args(**kw):
    from usdm_amd import _lib
    a = _lib.SnakeArgs()
    a.x, a.alpha, a.beta, a.out32, a.out16 = PTR, PTR, PTR, PTR, PTR
    a.T, a.C, a.Creal, a.L, a.ldx, a.ldo, a.logscale = 5, 34, 33, 0, 34, 34, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_usdm_aa_snake_refusals():
    """every refusal returns before anything is launched (the pointers here are not memory)"""
    from usdm_amd import _lib

    def refused(word, **kw):
        rc = _lib.lib.usdm_aa_snake(C_.byref(_args(**kw)), None)
        msg = _lib.lib.usdm_last_error()
        assert rc == 2 and word in msg, (kw, rc, msg)
    refused(b"bad T/C", C=33)
    refused(b"bad T/C", Creal=35)
    refused(b"bad T/C", T=0)
    refused(b"strides", ldx=35)
    refused(b"strides", ldo=35)
    refused(b"no output", out32=None, out16=None)
    for p in ("x", "alpha", "beta"):
        refused(b"null", **{p: None})
    refused(b"aligned", x=PTR + 4)
    refused(b"aligned", out32=PTR + 4)
    refused(b"aligned", out16=PTR + 2)
    refused(b"aligned", out32=None, out16=PTR + 2)
    refused(b"aligned", out32=PTR + 4, out16=None)
    assert _lib.lib.usdm_aa_snake(None, None) == 2
