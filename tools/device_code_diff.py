"""Compare the gfx950 device code of two csrc/ trees kernel by kernel: the check of a host-only refactor.
Every *.hip of both trees is compiled to assembly (hipcc cross-compiles without a GPU), split into kernels with
isa_events.kernels, and each kernel's body is compared as text after normalising the compiler's function-local label
numbering only (a label's number, and the padding in front of its comment, which follows the number's width).  Whole files
differ when launches move (instantiation order); the kernels must not.  Both trees sit in a checkout (`git worktree add`
gives the old one): the sources include ../../include/nvq.h.
usage: python tools/device_code_diff.py <old csrc> <new csrc> [-j N]      exit status 1 if any kernel differs"""
import argparse, concurrent.futures, os, re, shutil, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_events import kernels

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LABELS = [(re.compile(r"BB\d+_"), "BB_"), (re.compile(r"\.Lfunc_begin\d+"), ".Lfunc_begin"),
          (re.compile(r"\.Lfunc_end\d+"), ".Lfunc_end"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"),
          (re.compile(r"^(\.L\w+:)\s+;"), r"\1 ;")]


def normalise(line):
    for pat, rep in LABELS:
        line = pat.sub(rep, line)
    return line


def device_kernels(src, tmp):
    """{kernel symbol: normalised body} of one translation unit"""
    out = os.path.join(tmp, os.path.basename(src) + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-S", "--cuda-device-only",
                    src, "-o", out], check=True)
    return {name: "".join(normalise(l) for l in body) for name, body in kernels(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    names = sorted({f for d in (a.old, a.new) for f in os.listdir(d) if f.endswith(".hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new, \
            concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        jobs = {}
        for f in names:
            for d, t in ((a.old, t_old), (a.new, t_new)):
                p = os.path.join(d, f)
                jobs[d, f] = pool.submit(device_kernels, p, t) if os.path.exists(p) else None
        print(f"{'source':<20} {'old':>5} {'new':>5} {'identical':>9}")
        tot = [0, 0, 0]
        for f in names:
            old, new = (jobs[d, f].result() if jobs[d, f] else {} for d in (a.old, a.new))
            same = sum(1 for k in old if new.get(k) == old[k])
            print(f"{f:<20} {len(old):>5} {len(new):>5} {same:>9}")
            for k in sorted(set(old) | set(new)):
                what = "only in old" if k not in new else "only in new" if k not in old else \
                    "differs" if old[k] != new[k] else None
                if what:
                    bad += 1
                    print(f"    {what}: {k}")
            tot = [tot[0] + len(old), tot[1] + len(new), tot[2] + same]
        print(f"{'total':<20} {tot[0]:>5} {tot[1]:>5} {tot[2]:>9}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
