"""CPU: the hand-counted weight ring of gemv_stream_kernel (csrc/llm_k.hip; down_proj of the decode step, K = 14336), read in the
gfx950 assembly with the library's own flags (tools/check_mfma_asm.py, as tests/test_gemv_resident_asm_cpu.py does):
  * no compiler-generated instruction touches the destination of an asm load that is still in flight;
  * the loads are the 2 pieces of x + the first ring + one refill per consumed slot but the last ring's;
  * from the prologue's barrier to the last refill every vector-memory wait leaves the whole ring but its oldest load in flight -
    the ring never drains in the K loop - and after the last refill the count falls by one per consume;
  * four waves per SIMD (one 16-wave workgroup per CU) without scratch;
  * the launch selection picks the form at the 7B's down_proj and nowhere else by default."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIT, UNR = 28, 8
INST = f"gemv_stream_kernelILi{NIT}ELi{UNR}E"
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


def test_ring_is_clean_and_never_drains_in_the_k_loop(asm):
    t = _tool()
    (name, i0, i1), = t.kernels(asm, INST, whole=True)      # (the skip return is an s_endpgm in the prologue)
    nload, bad = t.audit(asm, i0, i1)
    assert not bad, bad[:5]
    assert nload == 2 + UNR + (NIT - UNR)
    code = [ln.split(";")[0] for ln in asm[i0:i1]]
    loads = [i for i, c in enumerate(code) if t.LOAD.search(c) and " nt" in c]
    assert len(loads) == nload - 2
    barriers = [i for i, c in enumerate(code) if "s_barrier" in c]
    assert len(barriers) == 1 and loads[UNR - 1] < barriers[0] < loads[UNR]   # one barrier, behind the first ring's issue
    # the prologue: no vector-memory wait in front of the ring's issue, then the one that names exactly UNR younger loads
    assert not [c for c in code[:loads[UNR - 1]] if VMWAIT.search(c)]
    pro = [int(m.group(1)) for c in code[loads[UNR - 1]:barriers[0]] if (m := VMWAIT.search(c))]
    assert pro == [UNR], pro
    waits = [int(m.group(1)) for c in code[barriers[0]:loads[-1]] if (m := VMWAIT.search(c))]
    assert len(waits) == NIT - UNR and set(waits) == {UNR - 1}, waits
    tail = [int(m.group(1)) for c in code[loads[-1]:] if (m := VMWAIT.search(c))]
    assert tail[:UNR] == list(range(UNR - 1, -1, -1)), tail       # one load fewer in flight per consume


def test_four_waves_per_simd_and_no_scratch(asm):
    text = "\n".join(asm)
    desc = text[text.index(".amdhsa_kernel _ZN12_GLOBAL__N_118" + INST):]
    desc = desc[:desc.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 128
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)) == 0
    assert f"{INST}EEv14usdm_gemv_args.private_seg_size, 0" in text


def test_selection_takes_the_form_at_down_proj_only():
    """usdm_gemv_streams / usdm_gemv_threads read the launch selection: the form has gemv_kernel<1, false, 16>'s workgroups, by
    default where the table picks them anyway, under resident > 0 at any N - at K = 14336, plain calls only"""
    from usdm_amd import _lib
    assert ctypes.sizeof(_lib.GemvArgs) == _lib.lib.usdm_sizeof_gemv_args()

    def sel(**kw):
        a = _lib.GemvArgs(**{"ldw": kw["K"], **kw})
        return _lib.lib.usdm_gemv_streams(ctypes.byref(a)), _lib.lib.usdm_gemv_threads(ctypes.byref(a))

    # the 7B's down_proj, then its o_proj: the same 16-wave workgroups, the new form by default in the first only
    assert sel(N=4096, K=14336) == (1, 1024) and sel(N=4096, K=14336, resident=-1) == (0, 1024)
    assert sel(N=4096, K=4096) == (0, 1024) and sel(N=4096, K=4096, resident=1) == (0, 1024)
    assert sel(N=4096, K=14336, ldw=14336 + 8) == (1, 1024)
    # shapes with a four-wave row of their own
    for n in (16, 40, 272):
        assert sel(N=n, K=14336) == (0, 256) and sel(N=n, K=14336, resident=-1) == (0, 256)     # not the default, nor -1
        assert sel(N=n, K=14336, resident=1) == (1, 1024)                                        # the override
        assert sel(N=n, K=4096, resident=1) == (0, 256) and sel(N=n, K=14336 + 512, resident=1) == (0, 256)      # another K: never
    # a call that is not plain keeps its kernel, default and override: fused RMSNorm, x_delta, lm_head mode, merged input, the
    # fused all-reduce, SwiGLU (the table only compares the pointers with null)
    for other in (dict(norm_w=64), dict(x_delta=64), dict(part_val=64), dict(mrg_po=64), dict(p2p_mode=1)):
        assert sel(N=40, K=14336, resident=1, **other) == (0, 256), other
        assert sel(N=4096, K=14336, **other)[0] == 0, other
    assert sel(N=64, K=14336, act=3, resident=1) == (0, 448) and sel(N=8192, K=14336, act=3)[0] == 0
