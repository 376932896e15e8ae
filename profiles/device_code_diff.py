#!/usr/bin/env python3
"""Which device functions does a change touch?  Compiles csrc/engine.hip of two source trees to gfx950 assembly (device code only,
the Makefile's flags; no GPU needed, ~30 s per tree) and lists the functions whose instruction streams differ:

    git worktree add /tmp/parent HEAD~1            # or: git archive HEAD~1 | tar -x -C /tmp/parent
    python profiles/device_code_diff.py /tmp/parent . [-DTS_LDS_HEAP=128 ...]

Arguments after the two trees go to the compiler of both (the Makefile's -D sets of the test builds, say).  Per function the
stream is its instructions and labels in order; comments, assembler directives, the function's number inside the .LBB labels and the
per-build __hip_cuid_* symbol are left out.  Prints one line per function that differs or exists in one tree only, with the
instruction counts, and exits 1 if there is any, 0 if every function is the same.  It compares two builds and nothing else: it
does not look at what the instructions are."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-pthread", "-Wno-unused-function", "--offload-arch=gfx950"]     # csrc/Makefile CXXFLAGS
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(tree, extra, out):
    csrc = os.path.join(os.path.abspath(tree), "trafficsimulation_amd", "csrc")
    subprocess.run([HIPCC, *extra, *FLAGS, "--cuda-device-only", "-S", "-o", out, "engine.hip"], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def functions(lines):
    """name -> [normalised instruction and label lines]"""
    types = {m.group(1) for l in lines for m in [re.match(r"\s*\.type\s+([^,\s]+),@function", l)] if m}
    out, cur = {}, None
    for l in lines:
        t = l.split(";", 1)[0].strip()
        if cur is None:
            if t.endswith(":") and t[:-1] in types:
                cur = out.setdefault(t[:-1], [])
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
            continue
        if not t or t.startswith("//") or (t.startswith(".") and not re.match(r"\.LBB\d+_\d+:", t)):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"__hip_cuid_\w+", "__hip_cuid", t)))
    return out


def short(name):    # (mangled names of the anonymous namespace: _ZN12_GLOBAL__N_1<len><name>...)
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


def n_inst(body):
    return sum(1 for t in body if not t.endswith(":"))


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a_tree, b_tree, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(2) as ex:
        fa = ex.submit(assembly, a_tree, extra, os.path.join(tmp, "a.s"))
        fb = ex.submit(assembly, b_tree, extra, os.path.join(tmp, "b.s"))
        a, b = functions(fa.result()), functions(fb.result())
    print("# %s -> %s%s: %d / %d functions" % (a_tree, b_tree, (" " + " ".join(extra)) if extra else "", len(a), len(b)))
    n = 0
    for name in sorted(set(a) | set(b), key=lambda s: (short(s), s)):
        if name in a and name in b:
            if a[name] == b[name]:
                continue
            first = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
            print("differs   %-24s %6d -> %6d instructions, first difference at line %d of the stream   %s" %
                  (short(name), n_inst(a[name]), n_inst(b[name]), first, name))
        elif name in a:
            print("only in A %-24s %6d instructions   %s" % (short(name), n_inst(a[name]), name))
        else:
            print("only in B %-24s %6d instructions   %s" % (short(name), n_inst(b[name]), name))
        n += 1
    print("# %d function%s differ%s" % (n, "" if n == 1 else "s", "s" if n == 1 else ""))
    return 1 if n else 0


if __name__ == "__main__":
    sys.exit(main())
