#!/usr/bin/env python3
"""Static instruction mix of the A* search loop (astar_loop in csrc/astar.h) in the gfx950 ISA, by class.  No GPU needed:

    python profiles/isa_mix.py [engine.s]          # without an argument: compiles csrc/engine.hip with -S first (~30 s)

astar_wave holds eight instantiations of the loop (<SPILL, HALF, FOV>).  Every loop of the function of 100 instructions
and more is listed with its nesting depth and class totals (a pair of SPILL forms sits inside the loop that switches between them); the default policy's fast form <false, true, false> is the one without f64 arithmetic (HALF), without
the field-of-view load (three vector-memory loads, not four) and without heap accesses to HBM (SPILL = false: the fewest
vector-memory instructions).  The figures are static: the instructions between a loop's head and its last back edge, cold
blocks (path reconstruction, the second sift-down window) included."""
import collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trafficsimulation_amd", "csrc")
if len(sys.argv) > 1:
    path = sys.argv[1]
else:
    path = os.path.join(tempfile.mkdtemp(), "engine.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-pthread", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    "-o", path, "engine.hip"], cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
lines = open(path).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"_ZN12_GLOBAL__N_110astar_wave.*:", l))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end]


def klass(op):
    if op.startswith("s_cbranch") or op == "s_branch":
        return "scalar_branch"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait_nop"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "scalar_mem"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "scratch" if op.startswith("scratch_") else "vmem"
    if op.startswith("v_"):
        return "vector"
    return "other"


label_at, insts = {}, []     # label -> index of the next instruction; (op, text)
for l in body:
    t = l.strip()
    m = re.match(r"(\.LBB\d+_\d+):", t)
    if m:
        label_at[m.group(1)] = len(insts)
        continue
    if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
        continue
    insts.append((t.split()[0], t))
back = []                    # (head, branch) instruction indices of backward branches
for i, (op, t) in enumerate(insts):
    if klass(op) == "scalar_branch":
        m = re.search(r"(\.LBB\d+_\d+)", t)
        if m and m.group(1) in label_at and label_at[m.group(1)] <= i:
            back.append((label_at[m.group(1)], i))
loops = {}                   # natural loops by head: head -> last back edge; nesting depth = loops that contain it
for h, b in back:
    loops[h] = max(loops.get(h, 0), b)
outer = sorted(([h, b] for h, b in loops.items() if b - h >= 100), key=lambda p: (p[0], -p[1]))
cols = ["scalar", "scalar_branch", "vector", "lds", "vmem", "scratch", "scalar_mem", "wait_nop"]
print("loop,depth,first_inst,last_inst," + ",".join(cols) + ",total_issued,f64,s_mov,saveexec")
for n, (h, b) in enumerate(outer):
    c = collections.Counter(klass(op) for op, _ in insts[h:b + 1])
    ops = [op for op, _ in insts[h:b + 1]]
    if c["lds"] < 4:
        continue             # (not a search loop: the table clear of next_epoch, the path copy)
    depth = sum(1 for h2, b2 in outer if h2 <= h and b2 >= b) - 1
    print(",".join([str(n), str(depth), str(h), str(b)] + [str(c[k]) for k in cols] +
                   [str(sum(c[k] for k in cols)), str(sum("f64" in o for o in ops)), str(sum(o.startswith("s_mov") for o in ops)),
                    str(sum("saveexec" in o for o in ops))]))
c = collections.Counter(klass(op) for op, _ in insts)
print("astar_wave,,0,%d," % len(insts) + ",".join(str(c[k]) for k in cols) + ",%d,,," % sum(c[k] for k in cols))
