"""CPU: the two hand-counted weight rings of gemv_stream_wpack_kernel (csrc/llm_k.hip; down_proj of the decode step over the
13-bit weight image), read in the gfx950 assembly with the library's own flags, in the manner of tests/test_gemv_down_asm_cpu.py:
  * along every control-flow path no compiler-generated instruction touches the destination of an asm load that is still in flight
    (tools/check_mfma_asm.py audit_paths: the kernel has two bodies, the packed rows' and the marked rows', and the walk agrees
    with the tool's linear scan on the two one-body kernels);
  * each body's loads are the 2 pieces of x + its first ring + one refill per consumed slot but the last ring's;
  * in each body, from its barrier to its last refill every vector-memory wait is a hand-counted one that leaves the whole ring but
    the consumed unit (slot) in flight, and after the last refill the count falls by one unit (slot) per consume;
  * four waves per SIMD without scratch."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIT, RU, UB = 28, 3, 12
NU = NIT // 4
INST = f"gemv_stream_wpack_kernelILi{NIT}ELi{RU}ELi{UB}E"
VMWAIT = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")


def _tool():
    spec = importlib.util.spec_from_file_location("check_mfma_asm", os.path.join(ROOT, "tools", "check_mfma_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from usdm_amd import build
    if not os.path.exists(build.HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("hipcc is not installed")
    hipcc = build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "llm_k.s")
    src = os.path.join(build.CSRC, "llm_k.hip")
    r = subprocess.run([hipcc, *build.FLAGS, *build.EXTRA.get("llm_k.hip", []), "--cuda-device-only", "-S", src, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read().split("\n")


def test_both_rings_are_clean_and_never_drain_in_the_k_loop(asm):
    t = _tool()
    (name, i0, i1), = t.kernels(asm, INST, whole=True)
    nload, bad = t.audit_paths(asm, i0, i1)
    assert not bad, bad[:5]
    assert nload == (2 + 4 * RU + 4 * (NU - RU)) + (2 + UB + (NIT - UB))         # both bodies were walked
    for one_body in ("gemv_stream_kernelILi28ELi8E", "gemv_resident_kernelILi2ELi7ELi2ELi8E"):
        (_, j0, j1), = t.kernels(asm, one_body, whole=True)
        assert t.audit_paths(asm, j0, j1) == t.audit(asm, j0, j1) and t.audit(asm, j0, j1)[0] > 0
    code = [ln.split(";")[0] for ln in asm[i0:i1]]
    nt = [i for i, c in enumerate(code) if t.LOAD.search(c) and " nt" in c]
    sign = [i for i in nt if re.search(r"global_load_dword\s", code[i])]           # only a packed unit has a one-dword load
    assert len(sign) == NU and len(nt) == 4 * NU + NIT
    barriers = [i for i, c in enumerate(code) if "s_barrier" in c]
    assert len(barriers) == 2
    seen = set()
    for b in barriers:
        # a body's K loop: from its barrier to its last consume, the first wait for everything (straight-line code)
        z = next(i for i in range(b, len(code)) if re.search(r"s_waitcnt vmcnt\(0\)", code[i]))
        refills = [i for i in nt if b < i < z]
        packed = any(i in sign for i in refills)
        seen.add(packed)
        # packed: units in flight, four loads each, one wait per unit; marked: gemv_stream_kernel's loop at depth UB
        depth, slots, per_slot = (RU, NU, 4) if packed else (UB, NIT, 1)
        assert len(refills) == per_slot * (slots - depth), (packed, len(refills))
        waits = [int(m.group(1)) for c in code[b:refills[-1]] if (m := VMWAIT.search(c))]
        assert waits == [per_slot * (depth - 1)] * (slots - depth), (packed, waits)
        tail = [int(m.group(1)) for c in code[refills[-1]:z + 1] if (m := VMWAIT.search(c))]
        assert tail == [per_slot * k for k in range(depth - 1, -1, -1)], (packed, tail)
    assert seen == {True, False}


def test_four_waves_per_simd_and_no_scratch(asm):
    text = "\n".join(asm)
    desc = text[text.index(".amdhsa_kernel _ZN12_GLOBAL__N_124" + INST):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 128
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0
    assert f"{INST}EEv14usdm_gemv_args15usdm_gemv_wpack.private_seg_size, 0" in text


def test_selection_takes_the_packed_form_where_the_stream_form_runs():
    """usdm_gemv_packs reads the launch selection: exactly the calls that usdm_gemv runs in the straight-line form"""
    import ctypes
    from usdm_amd import _lib

    def sel(**kw):
        a = _lib.GemvArgs(**{"ldw": kw["K"], **kw})
        return _lib.lib.usdm_gemv_packs(ctypes.byref(a)), _lib.lib.usdm_gemv_streams(ctypes.byref(a))

    assert sel(N=4096, K=14336) == (1, 1) and sel(N=4096, K=14336, resident=-1) == (0, 0)
    assert sel(N=4096, K=4096) == (0, 0) and sel(N=28672, K=4096, act=3) == (0, 0)
    for n in (16, 40, 272):
        assert sel(N=n, K=14336) == (0, 0) and sel(N=n, K=14336, resident=1) == (1, 1)
    for other in (dict(norm_w=64), dict(x_delta=64), dict(part_val=64), dict(mrg_po=64), dict(p2p_mode=1)):
        assert sel(N=4096, K=14336, **other) == (0, 0), other
