"""CPU: the two hand-counted weight rings of gemv_resident_wpack_kernel (csrc/llm_k.hip; gate/up of the decode step over the 13-bit
weight image), read in the gfx950 assembly with the library's own flags, in the manner of tests/test_gemv_packed_asm_cpu.py:
  * along every control-flow path no compiler-generated instruction touches the destination of an asm load that is still in flight
    (tools/check_mfma_asm.py audit_paths: the kernel has two bodies, the packed waves' and the marked waves');
  * each body's loads are the 3 early loads + its first ring + one refill per consumed unit (slot) but the last ring's;
  * in the packed body, from its last barrier to its last refill every vector-memory wait is a hand-counted one that leaves
    4 (RU - 1) loads in flight - through the seam of the two tiles - and after the last refill the count falls by four per unit;
  * in the marked body the waits are gemv_resident_kernel<2, 7, 2, 8>'s: vmcnt(15) in front of all 48 refilled consumes and the
    first of the tail, then 14 .. 0;
  * four waves per SIMD without scratch;
  * usdm_gemv_packs_glu answers what needs no device without one."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSEQ = 16          # units of a wave: 2 tiles x 2 units x 4 rows
NR, UNR, NIT, TPW = 4, 4, 8, 2
VMWAIT = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")


def _tool():
    spec = importlib.util.spec_from_file_location("check_mfma_asm", os.path.join(ROOT, "tools", "check_mfma_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ru():
    """the ring depth the library is built with (csrc/llm_k.hip USDM_GEMV_GU_WPACK_RU)"""
    src = open(os.path.join(ROOT, "usdm_amd", "csrc", "llm_k.hip")).read()
    return int(re.search(r"#define USDM_GEMV_GU_WPACK_RU (\d+)", src).group(1))


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


def test_both_rings_are_clean_and_never_drain_between_the_tiles(asm):
    t = _tool()
    RU = _ru()
    (name, i0, i1), = t.kernels(asm, f"gemv_resident_wpack_kernelILi{RU}E", whole=True)
    nload, bad = t.audit_paths(asm, i0, i1)
    assert not bad, bad[:5]
    assert nload == (3 + 4 * RU + 4 * (NSEQ - RU)) + (3 + NR * UNR + NR * (TPW * NIT - UNR))      # both bodies were walked
    code = [ln.split(";")[0] for ln in asm[i0:i1]]
    nt = [i for i, c in enumerate(code) if t.LOAD.search(c) and " nt" in c]
    sign = [i for i in nt if re.search(r"global_load_dword\s", code[i])]           # only a packed unit has a one-dword load
    assert len(sign) == NSEQ and len(nt) == 4 * NSEQ + NR * TPW * NIT
    barriers = [i for i, c in enumerate(code) if "s_barrier" in c]
    assert len(barriers) == 4             # per body: the RMSNorm statistic's and the one behind the staging, in equal number
    seen = set()
    for b in barriers[1::2]:
        # a body's tiles: from its last barrier to its last consume, the first wait for everything (straight-line code but for
        # the lane-0 stores of the first tile's epilogue)
        z = next(i for i in range(b, len(code)) if re.search(r"s_waitcnt vmcnt\(0\)", code[i]))
        assert not any(b < o < z for o in barriers)
        refills = [i for i in nt if b < i < z]
        packed = any(i in sign for i in refills)
        seen.add(packed)
        waits = [int(m.group(1)) for c in code[b:refills[-1]] if (m := VMWAIT.search(c))]
        tail = [int(m.group(1)) for c in code[refills[-1]:z + 1] if (m := VMWAIT.search(c))]
        if packed:
            assert len(refills) == 4 * (NSEQ - RU)
            assert waits == [4 * (RU - 1)] * (NSEQ - RU), waits
            assert tail == [4 * k for k in range(RU - 1, -1, -1)], tail
        else:
            assert len(refills) == NR * (TPW * NIT - UNR)
            assert waits == [NR * UNR - 1] * (NR * (TPW * NIT - UNR)), waits
            assert tail == list(range(NR * UNR - 1, -1, -1)), tail
    assert seen == {True, False}


def test_four_waves_per_simd_and_no_scratch(asm):
    text = "\n".join(asm)
    inst = f"gemv_resident_wpack_kernelILi{_ru()}E"
    desc = text[text.index(".amdhsa_kernel _ZN12_GLOBAL__N_126" + inst):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 128
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0
    assert f"{inst}EEv14usdm_gemv_args15usdm_gemv_wpack.private_seg_size, 0" in text


def test_the_query_needs_no_device_where_the_answer_is_no():
    """usdm_gemv_packs_glu is 1 exactly where gemv_launch_resident launches the straight-line instantiation; both read
    gemv_straight_form and the same grid rule (csrc/llm_k.hip).  Here, without a device: every call that is not a plain bf16 SwiGLU
    call on the resident row at K = 4096 is answered 0 before the device is asked; tests/test_gemv_gu_packed_gpu.py holds the
    table's other half (1 at two tiles per workgroup, 0 at every other cap).  usdm_gemv_packs keeps its own answer."""
    import ctypes
    from usdm_amd import _lib

    def sel(**kw):
        a = _lib.GemvArgs(**{"ldw": kw["K"], **kw})
        return _lib.lib.usdm_gemv_packs_glu(ctypes.byref(a)), _lib.lib.usdm_gemv_packs(ctypes.byref(a))

    assert sel(N=28672, K=4096, act=3, resident=-1) == (0, 0)            # the one-tile form asked for
    assert sel(N=28672, K=4096, act=0) == (0, 0) and sel(N=4096, K=14336) == (0, 1)
    assert sel(N=224, K=512, act=3, resident=4) == (0, 0) and sel(N=224, K=4104, act=3, resident=4) == (0, 0)
    assert sel(N=1024, K=4096, act=3) == (0, 0)                          # not the resident row, no cap given
    for other in (dict(x_delta=64), dict(x_delta=64, x_out=64), dict(x_out=64), dict(mrg_po=64), dict(p2p_mode=1)):
        assert sel(N=28672, K=4096, act=3, **other)[0] == 0, other
