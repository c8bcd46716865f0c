#!/usr/bin/env python3
"""Is the device code of two trees the same?  Compiles every csrc/*.hip of both trees to gfx950 assembly (the flags of
build.py plus -S --cuda-device-only), splits the text per kernel, normalises what a rename changes (the kernel's own mangled
name, the function number in local labels) and reports per kernel whether the instruction text is identical, with the
resource metadata of both sides.  For kernels that differ it also lists the counts of the instruction classes the hot loops
are built from.  CPU only (hipcc cross-compiles).

    python scripts/isa_compare.py OLD_TREE NEW_TREE [file.hip ...]       e.g. OLD_TREE = a `git worktree` of the parent commit
    python scripts/isa_compare.py --moved a.hip:old_kernel[:i]=b.hip:new_kernel[:j] [--moved ...] OLD_TREE NEW_TREE [file.hip ...]

Kernels are paired by (file, unqualified name without template arguments, position among the kernels of that name in the order
the compiler emits them), so an instantiation whose template parameter list was shortened still meets its predecessor; both
demangled names are printed for every pair that is not identical.  --moved pairs the first (or i-th, from 0) kernel of that name in one file of the
old tree with the first (or j-th) of the other name in a file of the new tree (a kernel that changed its file, its name or both) and
reports the pair under MOVED.  Exit status 1 when a kernel differs or has no partner.
"""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "image-search-engine-for-historical-research_amd"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
META = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
CLASSES = ("v_mfma", "s_barrier", "global_load_lds", "ds_", "s_waitcnt vmcnt")


def build_flags(tree):
    ns = {}
    src = open(os.path.join(tree, PKG, "build.py")).read()
    exec(re.search(r"^FLAGS = \[.*?\]$", src, re.M | re.S).group(0), ns)
    return ns["FLAGS"]


def compile_asm(tree, name, td):
    out = os.path.join(td, "%s_%s.s" % (abs(hash(tree)), name))
    cmd = [HIPCC, *build_flags(tree), "-S", "--cuda-device-only", "-o", out, os.path.join(tree, PKG, "csrc", name)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit("hipcc failed for %s of %s:\n%s" % (name, tree, r.stderr[-3000:]))
    return open(out).read()


def demangle(names):
    if not names or not CXXFILT:
        return list(names)
    return subprocess.run([CXXFILT, *names], capture_output=True, text=True).stdout.split("\n")[:len(names)]


def kernels_of(asm):
    """[(mangled, demangled, normalised instruction lines, metadata dict)] in emission order."""
    lines = asm.split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    meta = {}
    for entry in re.split(r"^  - (?=\.)", asm[asm.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        m = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        meta[m.group(1)] = {k: int(re.search(r"^\s*\.%s:\s*(\d+)" % k, entry, re.M).group(1)) for k in META}
    out = []
    for mangled, pretty in zip(names, demangle(names)):
        start = next(i for i, l in enumerate(lines) if l.startswith(mangled + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".section"))
        body = []
        for l in lines[start + 1:end]:
            l = l.split(";")[0].rstrip()
            if not l.strip() or l.strip().startswith(".p2align"):
                continue
            l = l.replace(mangled, "KERNEL")
            body.append(re.sub(r"\.L(BB|tmp|JTI)\d+_", r".L\1_", l))
        out.append((mangled, pretty, body, meta[mangled]))
    return out


def base_name(mangled):
    """Unqualified name of an Itanium-mangled function: the last <length><identifier> of its (nested) name."""
    i, name = (3 if mangled.startswith("_ZN") else 2), mangled
    while i < len(mangled) and mangled[i].isdigit():
        n = re.match(r"\d+", mangled[i:]).group(0)
        name = mangled[i + len(n):i + len(n) + int(n)]
        i += len(n) + int(n)
    return name


def compare(a, b, report):
    """1 when old kernel a and new kernel b are identical, else 0 with the differences appended to report."""
    if a[2] == b[2] and a[3] == b[3]:
        return 1
    report.append("  DIFFERS: %s\n       ->  %s\n    instructions %d -> %d" % (a[1], b[1], len(a[2]), len(b[2])))
    report.append("    " + "  ".join("%s %d -> %d" % (m, a[3][m], b[3][m]) for m in META))
    cnt = [collections.Counter(c for l in k[2] for c in CLASSES if c in l) for k in (a, b)]
    report.append("    " + "  ".join("%s %d -> %d" % (c, cnt[0][c], cnt[1][c]) for c in CLASSES))
    return 0


def main():
    args, moved = sys.argv[1:], []
    while args and args[0] == "--moved":
        moved.append([tuple(x.split(":")) for x in args[1].split("=")])
        args = args[2:]
    old, new = os.path.abspath(args[0]), os.path.abspath(args[1])
    files = args[2:] or sorted(set(f for t in (old, new) for f in os.listdir(os.path.join(t, PKG, "csrc")) if f.endswith(".hip")))
    differ = 0
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {(t, f): ex.submit(compile_asm, t, f, td) for f in files for t in (old, new)
                if os.path.exists(os.path.join(t, PKG, "csrc", f))}
        sides = {}
        for f in files:
            side = []
            for t in (old, new):
                keyed, seen = collections.OrderedDict(), collections.Counter()
                for k in (kernels_of(jobs[(t, f)].result()) if (t, f) in jobs else []):
                    b = base_name(k[0])
                    keyed[(b, seen[b])] = k
                    seen[b] += 1
                side.append(keyed)
            sides[f] = side
        at = lambda x: (x[1], int(x[2]) if len(x) > 2 else 0)   # noqa: E731
        moved = [(src, dst, sides[src[0]][0].pop(at(src)), sides[dst[0]][1].pop(at(dst))) for src, dst in moved]
        for f in files:
            side = sides[f]
            same = 0
            report = []
            for key in list(side[0]) + [k for k in side[1] if k not in side[0]]:
                a, b = side[0].get(key), side[1].get(key)
                if a is None or b is None:
                    differ += 1
                    report.append("  ONLY IN %s: %s" % ("OLD" if b is None else "NEW", (a or b)[1]))
                else:
                    same += compare(a, b, report)
                    differ += 1 - compare(a, b, [])
            print("%-22s %3d kernels identical (instruction text and metadata)%s" % (f, same, ", the others:" if report else ""))
            for r in report:
                print(r)
        for src, dst, a, b in moved:
            report = []
            ok = compare(a, b, report)
            differ += 1 - ok
            print("MOVED %s -> %s (%s): %s" % (":".join(src), ":".join(dst), b[1].split("(")[0], "identical (instruction text and metadata)" if ok else "NOT identical"))
            for r in report:
                print(r)
    print("RESULT: %s" % ("every kernel identical" if not differ else "%d kernels differ or have no partner" % differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
