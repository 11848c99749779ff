"""python tools/isa_compare.py <old tree> <new tree> [old=new ...] [-gone ...]: is the device code of two checkouts the same, kernel by kernel?

Every file of build.SOURCES is compiled device-only to gfx950 assembly in both trees (the flags of tools/isa_regs.sh).  Per
kernel: the descriptor's registers, LDS and scratch, and the instruction stream with comments and directives dropped,
basic-block labels renumbered and symbol names demangled without "(anonymous namespace)::" and "smx::" (the method of
profiles/recon_split_isa.txt).  Prints one line per kernel and the number that differ; needs no GPU.  A source file the old
tree does not have yet is compiled in the new tree alone and its kernels are listed as "new".  Kernels are matched by that
demangled name without its parameter list, across the files, so a parameter type that moved between namespaces is no rename and
a kernel that moved to another file is found there ("was ... in ..."); a kernel that was renamed or folded into another is
matched through an `old=new` argument (k_track_solve_rgbd=k_track_solve); where the new tree differs both trees' figures are
printed, and a kernel of the old tree that the new one no longer has is listed as "gone": it has to be named by a `-name`
argument, or the comparison fails ("GONE"), so that no kernel vanishes by accident."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from surfelmeshing_amd.build import SOURCES, _hipcc  # noqa: E402

STRIP = ("(anonymous namespace)::", "smx::")


def compile_to_asm(root, src, out):
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I", os.path.join(root, "include"),
           "-I", os.path.join(root, "surfelmeshing_amd", "csrc"), "-x", "hip", "--cuda-device-only", "-S",
           os.path.join(root, "surfelmeshing_amd", "csrc", src), "-o", out]
    return subprocess.Popen(cmd, stderr=subprocess.DEVNULL)


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    for s in STRIP:
        out = [o.replace(s, "") for o in out]
    return out[:len(names)]


def kernels(path):
    """{mangled name: ((vgpr, sgpr, lds, scratch), normalised stream, instruction count)} in file order."""
    s = open(path).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
        name, d = m.group(1), m.group(2)
        desc = tuple(int(re.search(k + r"\s+(\d+)", d).group(1)) for k in
                     (r"\.amdhsa_next_free_vgpr", r"\.amdhsa_next_free_sgpr", r"\.amdhsa_group_segment_fixed_size",
                      r"\.amdhsa_private_segment_fixed_size"))
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), s, re.S | re.M).group(1)
        lines = [re.sub(r"\s*;.*$", "", ln).strip() for ln in body.split("\n")]
        text = "\n".join(ln for ln in lines if ln and not (ln.startswith(".") and not ln.endswith(":")))
        labels = {}
        for lab in re.findall(r"\.LBB\d+_\d+", text):
            labels.setdefault(lab, ".L%d" % len(labels))
        text = re.sub(r"\.LBB\d+_\d+", lambda mm: labels[mm.group(0)], text)
        syms = sorted(set(re.findall(r"_Z\w+", text)), key=len, reverse=True)
        for sym, plain in zip(syms, demangle(syms) if syms else []):
            text = text.replace(sym, plain)
        res[name] = (desc, text, sum(1 for ln in text.split("\n") if not ln.endswith(":")))
    return res


def by_plain_name(k):
    return {re.sub(r"\(.*$", "", p).replace("void ", ""): k[n] for n, p in zip(k, demangle(list(k)) if k else [])}


def main(old, new, renames, may_go):
    tmp = tempfile.mkdtemp(prefix="isa_compare_")
    jobs = []
    for src in SOURCES:
        outs = [os.path.join(tmp, "%s_%s.s" % (tag, src)) for tag in ("old", "new")]
        have = [os.path.exists(os.path.join(root, "surfelmeshing_amd", "csrc", src)) for root in (old, new)]
        jobs.append((src, outs, [compile_to_asm(root, src, out) if h else None for root, out, h in zip((old, new), outs, have)]))
    print("%-70s %-18s %5s %5s %6s %7s %7s  %s" % ("kernel", "file", "vgpr", "sgpr", "lds", "scratch", "instrs", "verdict"))
    was, now = {}, []                       # old: plain name -> (file, kernel); new: (plain name, file, kernel) in file order
    for src, outs, procs in jobs:
        if any(p is not None and p.wait() != 0 for p in procs) or procs[1] is None:
            raise SystemExit("hipcc failed on " + src)
        if procs[0] is not None:
            was.update({name: (src, k) for name, k in by_plain_name(kernels(outs[0])).items()})
        now += [(name, src, k) for name, k in by_plain_name(kernels(outs[1])).items()]
    back = {n: o for o, n in renames.items()}
    total, differ, row = len(was), 0, "%-70s %-18s %5d %5d %6d %7d %7d  %s"
    for n, src, k in now:
        o = back.get(n, n)
        if o not in was:
            print(row % (n[:70], src, *k[0], k[2], "new"))
            continue
        old_src, ko = was.pop(o)
        same = ko[:2] == k[:2]
        differ += not same
        moved = ", was %s in %s" % (o, old_src) if (o, old_src) != (n, src) else ""
        if not same:
            print(row % ((o + " (old tree)")[:70], old_src, *ko[0], ko[2], ""))
        print(row % (n[:70], src, *k[0], k[2], ("identical" if same else "DIFFERS") + moved))
    lost = [o for o in was if o not in may_go]
    for o, (old_src, ko) in was.items():
        print(row % ((o + " (old tree)")[:70], old_src, *ko[0], ko[2], "GONE" if o in lost else "gone"))
    shutil.rmtree(tmp)
    print("%d kernels of the old tree, %d differ, %d gone (%d not named)" % (total, differ, len(was), len(lost)))
    return 1 if differ or lost else 0


if __name__ == "__main__":
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), dict(a.split("=") for a in sys.argv[3:] if not a.startswith("-")),
                  {a[1:] for a in sys.argv[3:] if a.startswith("-")}))
