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


def audit_paths(lines, i0, i1):
    """audit() along the control-flow paths of a kernel with more than one body (gemv_stream_wpack_kernel: the packed and the bf16
    rows).  The compiler merges the bodies' returns and the shared epilogue into blocks that are entered under FLAGS - scalar
    register pairs it sets to the constants 0 and -1 (s_mov_b64) and tests as `s_and_b64 vcc, exec, flag` + s_cbranch_vccz / vccnz -
    so a linear scan reads the epilogue as code under one body's ring, and a walk that takes both sides of those branches runs
    from one body into the other.  This walk keeps the constant flags it has seen set: a branch on a known flag is followed one
    way, every other conditional branch both ways; s_branch is followed, s_endpgm ends a path, a state is walked once.
    A flag is also tested as `s_and_saveexec_b64 saved, flag` + s_cbranch_execz / execnz (gemv_resident_wpack_kernel: the skip
    return enters the merged last store that way, under a zero flag): exec is then known to be zero until it is written again.
    -> (asm load instructions seen, [(line offset, code)] as audit())"""
    label = {m.group(1): i for i in range(i0, i1) if (m := re.match(r"(\.LBB\d+_\d+):", lines[i]))}
    seen, bad, loads = set(), {}, set()
    stack = [(i0, (), (), None, False)]
    while stack:
        # flags: known constant s[a:b]; vcc: True = known non-zero, False = known zero; execz: exec is known to be zero
        i, fifo, flags, vcc, execz = stack.pop()
        fifo, flags, inasm = list(fifo), dict(flags), False
        while i < i1:
            code = lines[i].split(";")[0]
            if re.match(r"\.LBB\d+_\d+:", lines[i]):
                key = (i, tuple(fifo), tuple(sorted(flags.items())), vcc, execz)
                if key in seen:
                    break
                seen.add(key)
            if "ASMSTART" in lines[i]:
                inasm = True
            elif "ASMEND" in lines[i]:
                inasm = False
            elif inasm:
                if LOAD.search(code):
                    fifo.append(frozenset(regs(REG.findall(code)[0])))
                    loads.add(i)
                m = re.search(r"s_waitcnt vmcnt\((\d+)\)", code)
                if m:
                    fifo = trim(fifo, int(m.group(1)))
            else:
                used = set()
                for tok in REG.findall(code):
                    used |= regs(tok)
                if any(used & f for f in fifo):
                    bad[i - i0] = code.strip()
                if re.search(r"\b(global|buffer|scratch|flat)_(load|store|atomic)", code):
                    fifo.append(frozenset())
                m = re.search(r"s_waitcnt.*vmcnt\((\d+)\)", code)
                if m:
                    fifo = trim(fifo, int(m.group(1)))
                if "s_endpgm" in code:
                    break
                # the constant flags: what writes a scalar pair or vcc either sets a known constant or ends the knowledge
                ops = re.match(r"\s*(\w+)\s+([^,\s]+)(?:,\s*([^,\s]+))?(?:,\s*([^,\s]+))?", code)
                if ops and not ops.group(1).startswith(("s_cbranch", "s_branch", "s_cmp", "s_waitcnt", "s_nop", "s_barrier")):
                    op, dst, a, b = ops.groups()
                    if dst == "exec" or "saveexec" in op:
                        execz = op == "s_and_saveexec_b64" and flags.get(a) == 0
                    if dst == "vcc" or op.startswith("v_cmp") and "_e64" not in op:
                        known = op in ("s_and_b64", "s_andn2_b64") and a == "exec" and b in flags
                        vcc = (bool(flags[b]) == (op == "s_and_b64")) if known else None    # (exec is not zero where a wave runs)
                    elif dst in flags or (op == "s_mov_b64" and re.match(r"s\[\d+:\d+\]$", dst)):
                        flags.pop(dst, None)
                        if op == "s_mov_b64" and a in ("0", "-1"):
                            flags[dst] = int(a)
                    m2 = re.match(r"s\[(\d+):(\d+)\]$", dst) or re.match(r"s(\d+)()$", dst)
                    if m2:      # a write that overlaps a flag pair under another name
                        lo, hi = int(m2.group(1)), int(m2.group(2) or m2.group(1))
                        for k in [k for k in flags if k != dst]:
                            ka, kb = map(int, re.match(r"s\[(\d+):(\d+)\]", k).groups())
                            if lo <= kb and ka <= hi:
                                del flags[k]
                m = re.match(r"\s*(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)", code)
                if m and m.group(1) == "s_branch":
                    i = label[m.group(2)]
                    continue
                if m:
                    taken = {"s_cbranch_vccz": vcc is not True, "s_cbranch_vccnz": vcc is not False,
                             "s_cbranch_execnz": not execz}.get(m.group(1), True)
                    falls = {"s_cbranch_vccz": vcc is not False, "s_cbranch_vccnz": vcc is not True,
                             "s_cbranch_execz": not execz}.get(m.group(1), True)
                    if taken and falls:
                        stack.append((label[m.group(2)], tuple(fifo), tuple(flags.items()), vcc, execz))
                    elif taken:
                        i = label[m.group(2)]
                        continue
            i += 1
    return len(loads), sorted(bad.items())


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
