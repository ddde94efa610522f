"""Audit of the hand-counted load streams of gemv_mfma_kernel (cdna_hip_programming.md 5.7 item 4): while an asm load is in flight
(issued by an asm statement, not yet covered by an asm `s_waitcnt vmcnt(N)` - in-order completion: a wait leaves the N youngest in
flight), NO compiler-generated instruction may read or write its destination registers (a copy, spill or reuse of a register whose
load has not landed is silent corruption).  Linear scan of the kernel's code; the stream loops keep the invariant from iteration to
iteration.  Usage: python tools/check_mfma_asm.py <file.s> [kernel-name-regex ...]
(tests/test_asm_audit_cpu.py runs it over every gemv_mfma_kernel instantiation with an asm load.)"""
import re
import sys

DEFAULT_PATS = [r"gemv_mfma_kernelILb1ELi16ELb0E", r"gemv_mfma_kernelILb1ELi16ELb1E"]
# every vector-memory load that writes VGPRs: global_load_dword / _dwordx2 / x3 / x4, the sub-dword forms and the d16 halves
LOAD = re.compile(r"\bglobal_load_(dword(x[234])?|[su]byte|[su]short|ubyte_d16\w*|sbyte_d16\w*|short_d16\w*)\b")
REG = re.compile(r"v\[\d+:\d+\]|v\d+\b")


def regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def trim(fifo, n):
    """what an `s_waitcnt vmcnt(n)` leaves in flight: the n youngest (all of them when n >= len)"""
    return fifo[-n:] if n else []


def kernels(lines, pat, whole=False):
    """(name, first line, s_endpgm line) of every function whose label matches pat; whole: up to the function's end label instead
    (a kernel with an early exit has its first s_endpgm in the prologue: gemv_stream_kernel's skip return)"""
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"(_Z\S*" + pat + r"\S*):", l)
        if m:
            end = ".Lfunc_end" if whole else "s_endpgm"
            i1 = next(j for j in range(i, len(lines)) if end in lines[j])
            out.append((m.group(1), i, i1))
    return out


def audit(lines, i0, i1):
    """(asm loads, [(line offset, code) of compiler instructions touching an in-flight asm destination])"""
    fifo, inasm, bad, nload = [], False, [], 0
    for i in range(i0, i1):
        code = lines[i].split(";")[0]
        if "ASMSTART" in lines[i]:
            inasm = True
        elif "ASMEND" in lines[i]:
            inasm = False
        elif inasm:
            if LOAD.search(code):
                fifo.append(regs(REG.findall(code)[0]))
                nload += 1
            m = re.search(r"s_waitcnt vmcnt\((\d+)\)", code)
            if m:
                fifo = trim(fifo, int(m.group(1)))
        else:
            used = set()
            for tok in REG.findall(code):
                used |= regs(tok)
            if any(used & f for f in fifo):
                bad.append((i - i0, code.strip()))
            # compiler-issued vector memory operations and waits move the same in-order counter (kernels that mix both kinds)
            if re.search(r"\b(global|buffer|scratch|flat)_(load|store|atomic)", code):
                fifo.append(set())
            m = re.search(r"s_waitcnt.*vmcnt\((\d+)\)", code)
            if m:
                fifo = trim(fifo, int(m.group(1)))
    return nload, bad


def main(argv):
    lines = open(argv[1]).read().split("\n")
    rc = 0
    for pat in argv[2:] or DEFAULT_PATS:
        for name, i0, i1 in kernels(lines, pat):
            nload, bad = audit(lines, i0, i1)
            print(f"{name}: {nload} asm loads; compiler instructions that touch a register while its asm load is in flight: {len(bad)}")
            for b in bad[:20]:
                print("  ", b)
            rc |= 1 if bad else 0
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv))
