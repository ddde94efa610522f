#!/usr/bin/env python3
"""Compares the gfx950 device code of .hip files between two source trees, function by function (CPU only: hipcc, no GPU).

    python tools/isa_diff.py TREE_A TREE_B llm_k.hip llm_batch_k.hip [--rename 9gemvb_mx4=8gemv_mx4] [--keep DIR] [--classify]

TREE_A / TREE_B are checkouts of this repository (each file is compiled from TREE/usdm_amd/csrc with usdm_amd.build.FLAGS plus
build.EXTRA, --cuda-device-only -S) or directories that already hold NAME.s for every NAME.hip listed.  The assembly is split into
functions; comments and assembler directives are dropped, and basic-block label numbers and the function's own name are normalised.
The kernel descriptor's .amdhsa_ lines (registers, scratch, LDS) are kept as part of the body, so a change of resources shows up as a
difference even where the instructions agree.

--rename OLD=NEW replaces OLD by NEW in the mangled names of A before matching (a type that changed its name, as the MXFP4 argument
struct did when the two GEMV files began to share it).  Exit status 1 if any function differs or exists on one side only.

--classify sorts every matched function into one of three classes instead (exit status 1 only for functions on one side only):
  A  identical after the normalisation above;
  B  same schedule: the .amdhsa_ lines, the multiset of mnemonics and the ordered sequence of memory instructions and s_waitcnt
     (mnemonic, wait counts / cache-policy words) are equal - only register numbers and commutative operand order differ;
  C  anything else; the changed descriptor lines, the waves per SIMD the register counts allow and the mnemonic-count delta follow.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from usdm_amd import build  # noqa: E402

MAX_JOBS = 16
LABEL = re.compile(r"\.L(BB|tmp|JTI|func_begin|func_end)\d+(_\d+)?")


def compile_asm(tree, files, outdir):
    """TREE/usdm_amd/csrc/NAME.hip -> outdir/NAME.s for every file"""
    os.makedirs(outdir, exist_ok=True)

    def one(f):
        src = os.path.join(tree, "usdm_amd", "csrc", f)
        out = os.path.join(outdir, f[:-4] + ".s")
        r = subprocess.run([build.HIPCC, *build.FLAGS, *build.EXTRA.get(f, []), "--cuda-device-only", "-S", src, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")

    with ThreadPoolExecutor(max_workers=max(1, min(MAX_JOBS, os.cpu_count() or 1, len(files)))) as ex:
        list(ex.map(one, files))
    return outdir


def functions(text):
    """{mangled name: normalised body lines} of one .s file"""
    lines = text.split("\n")
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", ln))]
    out = {}
    for name in names:
        i0 = lines.index(name + ":") if name + ":" in lines else next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        i1 = next(i for i in range(i0, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        body = []
        for ln in lines[i0 + 1:i1]:
            ln = ln.split(";")[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":") and not ln.startswith(".amdhsa_")):
                continue
            ln = LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln)
            body.append(re.sub(r"\s+", " ", ln.replace(name, "<self>")))
        out[name] = body
    return out


MEMORY = ("global", "flat", "buffer", "tbuffer", "scratch", "ds")   # first word of a vector-memory / LDS mnemonic
POLICY = {"nt", "sc0", "sc1", "glc", "slc", "dlc", "lds"}


def _split(body):
    """(descriptor lines, instruction lines) of a normalised body"""
    desc = [ln for ln in body if ln.startswith(".amdhsa_")]
    return desc, [ln for ln in body if not ln.startswith(".") and not ln.endswith(":")]


def _mnemonics(ins):
    out = {}
    for ln in ins:
        m = ln.split(" ", 1)[0]
        out[m] = out.get(m, 0) + 1
    return out


def _memory_sequence(ins):
    """ordered (mnemonic, wait counts or cache-policy words) of the memory instructions and waits"""
    seq = []
    for ln in ins:
        m, _, rest = ln.partition(" ")
        if m == "s_waitcnt":
            seq.append((m, rest.strip()))
        elif m.split("_", 1)[0] in MEMORY or m.startswith(("s_load", "s_buffer_load")):
            seq.append((m, " ".join(w for w in rest.replace(",", " ").split() if w in POLICY)))
    return seq


def _waves_per_simd(desc):
    """occupancy step of a gfx950 kernel: 512 unified registers per lane, allocated in blocks of 8, at most 8 waves"""
    for ln in desc:
        if ln.startswith(".amdhsa_next_free_vgpr "):
            n = max(1, int(ln.split()[1]))
            return min(8, 512 // (-(-n // 8) * 8))
    return None


def classify(a, b):
    """("A" | "B" | "C", report lines) of two normalised bodies"""
    if a == b:
        return "A", []
    (da, ia), (db, ib) = _split(a), _split(b)
    ma, mb = _mnemonics(ia), _mnemonics(ib)
    if da == db and ma == mb and _memory_sequence(ia) == _memory_sequence(ib):
        return "B", []
    rep = [f"{x}  ->  {y}" for x, y in zip(da, db) if x != y]
    if len(da) != len(db):
        rep.append(f"{len(da)} -> {len(db)} descriptor lines")
    rep.append(f"waves per SIMD {_waves_per_simd(da)} -> {_waves_per_simd(db)}")
    delta = {m: mb.get(m, 0) - ma.get(m, 0) for m in sorted(set(ma) | set(mb)) if ma.get(m, 0) != mb.get(m, 0)}
    rep.append("mnemonics: " + (", ".join(f"{m} {d:+d}" for m, d in delta.items()) or "same counts")
               + ("; memory / wait sequence differs" if _memory_sequence(ia) != _memory_sequence(ib) else "; memory / wait sequence equal"))
    return "C", rep


def classify_file(sa, sb, renames):
    """({name: (class, report)}, only in A, only in B) of one file's two assemblies"""
    fa, fb = functions(sa), functions(sb)
    out = {n: classify(body, fb[_apply(n, renames)]) for n, body in fa.items() if _apply(n, renames) in fb}
    matched = {_apply(n, renames) for n in fa}
    return out, [n for n in fa if n not in out], [n for n in fb if n not in matched]


def _apply(name, renames):
    for old, repl in renames:
        name = name.replace(old, repl)
    return name


def diff_file(sa, sb, renames):
    """(identical, renamed, different, only in A, only in B) name lists of one file's two assemblies"""
    fa, fb = functions(sa), functions(sb)
    same, renamed, differ, only_a = [], [], [], []
    for name, body in fa.items():
        new = _apply(name, renames)
        if new not in fb:
            only_a.append(name)
        elif body != fb[new]:
            differ.append(name)
        else:
            (renamed if new != name else same).append(name)
    matched = {_apply(n, renames) for n in fa}
    only_b = [n for n in fb if n not in matched]
    return same, renamed, differ, only_a, only_b


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("files", nargs="+", help=".hip file names under usdm_amd/csrc")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--keep", metavar="DIR", help="keep the compiled assembly under DIR/a and DIR/b")
    ap.add_argument("--classify", action="store_true", help="print class A / B / C per function (see above)")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        dirs = []
        for side, d in (("a", args.a), ("b", args.b)):
            is_tree = os.path.isdir(os.path.join(d, "usdm_amd", "csrc"))
            dirs.append(compile_asm(d, args.files, os.path.join(work, side)) if is_tree else d)
        bad = 0
        for f in args.files:
            sa, sb = (open(os.path.join(d, f[:-4] + ".s")).read() for d in dirs)
            if args.classify:
                cls, only_a, only_b = classify_file(sa, sb, renames)
                count = {c: sum(1 for k, _ in cls.values() if k == c) for c in "ABC"}
                print(f"{f}: {count['A']} class A, {count['B']} class B, {count['C']} class C, {len(only_a)} only in A, {len(only_b)} only in B")
                for n, (k, rep) in cls.items():
                    print(f"  {k} {n}")
                    for ln in rep:
                        print(f"      {ln}")
                for tag, ns in (("ONLY IN A", only_a), ("ONLY IN B", only_b)):
                    for n in ns:
                        print(f"  {tag} {n}")
                bad += len(only_a) + len(only_b)
                continue
            same, renamed, differ, only_a, only_b = diff_file(sa, sb, renames)
            print(f"{f}: {len(same) + len(renamed)} device functions identical ({len(renamed)} of them renamed), "
                  f"{len(differ)} different, {len(only_a)} only in A, {len(only_b)} only in B")
            for tag, ns in (("DIFFERENT", differ), ("ONLY IN A", only_a), ("ONLY IN B", only_b)):
                for n in ns:
                    print(f"  {tag} {n}")
            bad += len(differ) + len(only_a) + len(only_b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
