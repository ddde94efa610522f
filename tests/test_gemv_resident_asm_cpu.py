"""CPU: the hand-counted weight ring of gemv_resident_kernel's straight-line instantiation (csrc/llm_k.hip), read in the gfx950
assembly with the library's own flags (tools/check_mfma_asm.py, as tests/test_asm_audit_cpu.py does for gemv_mfma_kernel):
  * no compiler-generated instruction touches the destination of an asm load that is still in flight;
  * the ring is 3 early loads + the first ring + one refill per consumed slot but the last tile's last ring;
  * from the end of the prologue to the last refill - across the tile seam - every wait leaves the whole ring but its oldest load
    in flight: nothing drains between the K loops of consecutive tiles;
  * both instantiations fit four waves per SIMD (two 7-wave workgroups per CU) without scratch."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NR, UNR, TPW, NIT = 4, 4, 2, 8
STRAIGHT = f"gemv_resident_kernelILi2ELi7ELi{TPW}ELi{NIT}E"


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


def test_ring_is_clean_and_never_drains_at_the_seam(asm):
    t = _tool()
    (name, i0, i1), = t.kernels(asm, STRAIGHT)
    nload, bad = t.audit(asm, i0, i1)
    assert not bad, bad[:5]
    assert nload == 3 + NR * UNR + NR * (TPW * NIT - UNR)
    code = [ln.split(";")[0] for ln in asm[i0:i1]]
    loads = [i for i, c in enumerate(code) if t.LOAD.search(c) and " nt" in c]
    assert len(loads) == nload - 3
    start = [i for i, c in enumerate(code) if "s_barrier" in c][-1]      # x is staged: the K loop of the first tile begins
    waits = [int(m.group(1)) for c in code[start:loads[-1]] if (m := re.search(r"s_waitcnt.*vmcnt\((\d+)\)", c))]
    assert len(waits) == NR * (TPW * NIT - UNR) and set(waits) == {NR * UNR - 1}, waits
    tail = [int(m.group(1)) for c in code[loads[-1]:] if (m := re.search(r"s_waitcnt.*vmcnt\((\d+)\)", c))]
    assert tail[:NR * UNR] == list(range(NR * UNR - 1, -1, -1)), tail       # the last tile's tail: one load fewer per consume


def test_override_selects_the_14_output_tile_and_keeps_the_struct():
    """usdm_gemv_args.resident sits in what was tail padding (the last field before it is an int32 behind a pointer); non-zero selects
    the 7-wave tile at any SwiGLU shape, zero leaves the table as it was"""
    import ctypes
    from usdm_amd import _lib
    assert _lib.GemvArgs.resident.offset == _lib.GemvArgs.cmb_timeout_ms.offset + 4 and _lib.GemvArgs.resident.offset % 8 == 4
    assert ctypes.sizeof(_lib.GemvArgs) == _lib.GemvArgs.resident.offset + 4 == _lib.lib.usdm_sizeof_gemv_args()
    threads = lambda **kw: _lib.lib.usdm_gemv_threads(ctypes.byref(_lib.GemvArgs(K=512, ldw=512, act=3, **kw)))
    assert threads(N=192) == 256 and threads(N=192, resident=-1) == 448 and threads(N=192, resident=3) == 448
    assert threads(N=28672) == 448 and threads(N=28672, resident=-1) == 448


def test_resident_kernels_keep_two_workgroups_per_cu(asm):
    text = "\n".join(asm)
    for inst in (STRAIGHT, "gemv_resident_kernelILi2ELi7ELi0ELi0E"):
        desc = text[text.index(".amdhsa_kernel _ZN12_GLOBAL__N_120" + inst):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 128, inst
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0, inst
