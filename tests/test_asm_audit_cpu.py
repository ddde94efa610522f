"""CPU: the hand-counted load streams of gemv_mfma_kernel (csrc/llm_mfma_k.hip), bf16 and FP8, audited in the gfx950 assembly.

Their safety rests on hipcc's register allocation: no compiler-generated instruction may touch the destination of an asm load that is
still in flight (tools/check_mfma_asm.py).  The assembly is compiled here, device only, with the library's own flags, so a compiler
or source change that breaks the invariant fails the suite instead of corrupting results silently."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    out = str(tmp_path_factory.mktemp("asm") / "llm_mfma_k.s")
    src = os.path.join(build.CSRC, "llm_mfma_k.hip")
    r = subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(out).read().split("\n")


def _streams(t, lines):
    """every gemv_mfma_kernel instantiation that holds an asm load: (name, first line, end line)"""
    out = []
    for name, i0, i1 in t.kernels(lines, "gemv_mfma_kernel"):
        if any("ASMSTART" in lines[i] and t.LOAD.search(lines[i + 1].split(";")[0]) for i in range(i0, i1 - 1)):
            out.append((name, i0, i1))
    return out


def test_every_hand_counted_stream_is_clean(asm):
    t = _tool()
    ks = _streams(t, asm)
    names = [n for n, _, _ in ks]
    # bf16: the three row-contiguous forms and the fragment-shaped K = 4096 one; FP8: the three row-contiguous forms
    assert len(ks) == 7, names
    assert sum("ELb1EJPKa" in n for n in names) == 3, names
    for name, i0, i1 in ks:
        nload, bad = t.audit(asm, i0, i1)
        assert nload > 0, name
        assert not bad, (name, bad[:5])


def test_audit_catches_a_seeded_violation(asm):
    """a copy out of a register whose load is still in flight, inserted right behind the first hand-counted load of each stream"""
    t = _tool()
    for name, i0, i1 in _streams(t, asm):
        lines = list(asm)
        j = next(i for i in range(i0, i1) if "ASMSTART" in lines[i] and t.LOAD.search(lines[i + 1].split(";")[0]))
        dst = t.REG.findall(lines[j + 1].split(";")[0])[0]
        r0 = min(t.regs(dst))
        end = next(i for i in range(j, i1) if "ASMEND" in lines[i])
        lines.insert(end + 1, f"\tv_mov_b32_e32 v255, v{r0}")
        _, bad = t.audit(lines, i0, i1 + 1)
        assert bad and bad[0][1] == f"v_mov_b32_e32 v255, v{r0}", name


def test_fifo_keeps_everything_when_the_wait_allows_more_than_are_in_flight():
    t = _tool()
    fifo = [{1}, {2}, {3}]
    assert t.trim(fifo, 5) == fifo and t.trim(fifo, 3) == fifo      # (the old trim kept only the last 1 / all of them)
    assert t.trim(fifo, 2) == [{2}, {3}] and t.trim(fifo, 0) == []
    loads = {"global_load_dword v1, v[2:3], off": {1}, "global_load_dwordx2 v[4:5], v[2:3], off": {4, 5},
             "global_load_dwordx3 v[4:6], v[2:3], off": {4, 5, 6}, "global_load_dwordx4 v[4:7], v[2:3], off nt": {4, 5, 6, 7},
             "global_load_sbyte v9, v[2:3], off": {9}, "global_load_ushort v9, v[2:3], off": {9}}
    for op, dst in loads.items():
        assert t.LOAD.search(op), op
        assert t.regs(t.REG.findall(op)[0]) == dst, op
