"""The host searcher (csrc/astar_host.h: the wave searcher's algorithm as a sequential host function, and its thread pool) on the CPU:
tests/native/astar_host_check.cpp runs the 520 queries of tests/golden/astar_kats.npz - once single-threaded, eight times each on a
pool of four threads - and every path must equal the reference's cell for cell.  The A* snapshot words it searches on are built
here in numpy from their documented layout (the comment in csrc/astar_words.h; this restatement is the independent check and
does not read that header).  The program is built and run
three times: plain, under AddressSanitizer + UndefinedBehaviorSanitizer, and under ThreadSanitizer, as a plain executable."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "astar_host_check.cpp")
INC = os.path.join(HERE, "..", "trafficsimulation_amd", "csrc")
HDRS = [os.path.join(INC, h) for h in ("astar_host.h", "astar_words.h", "arena_epochs.h", "path_words.h")]
BUILD = os.path.join(HERE, "native", "_build")
GOLDEN = os.path.join(HERE, "golden")

# ts_default_params, in half units
TURN2, CONTRA2, VEH_PEN, STOP2, RT2, DYN_SCALE = 20, 10000, 1000.0, 1000, (1, 10, 100), 4.0
PEN_SHIFT = 10
LDS_HEAP = 704


def amap_words(allowed, is_road, road_type, inter, occ, stop, density32):
    """(snapshot words in 8 x 8-tiled order, number of search nodes) of one world, as k_world_cells + k_amap_build make them."""
    H, W = is_road.shape
    allowed = allowed.astype(np.uint32) & 15
    road = is_road == 1
    # nodes: the cells a search can stand on - roads, cells with flow bits, cells a flow bit points at (0: +y, 1: +x, 2: -y, 3: -x)
    node = road | (allowed != 0)
    node[1:, :] |= (allowed[:-1, :] & 1) != 0
    node[:, 1:] |= (allowed[:, :-1] & 2) != 0
    node[:-1, :] |= (allowed[1:, :] & 4) != 0
    node[:, :-1] |= (allowed[:, 1:] & 8) != 0
    flags = allowed | (road.astype(np.uint32) << 4) | ((inter == 1).astype(np.uint32) << 5) | ((road_type.astype(np.uint32) & 3) << 6)
    flags |= ((occ == 1).astype(np.uint32) << 8) | ((stop == 1).astype(np.uint32) << 9)
    pen2 = 2 * np.trunc(VEH_PEN * (1.0 + DYN_SCALE * density32.astype(np.float64))).astype(np.int64)
    assert pen2.max() < (1 << 22)
    flags |= pen2.astype(np.uint32) << PEN_SHIFT
    W8, H8 = (W + 7) // 8, (H + 7) // 8
    y, x = np.mgrid[0:H, 0:W]
    tix = ((((y >> 3) * W8 + (x >> 3)) << 6) | ((y & 7) << 3) | (x & 7)).astype(np.int64)
    # node numbers in tiled order
    order = np.argsort(tix[node], kind="stable")
    num = np.full((H, W), 0xFFFFFFFF, dtype=np.uint64)
    ny, nx = np.nonzero(node)
    num[ny[order], nx[order]] = np.arange(len(order), dtype=np.uint64)
    words = np.full(W8 * H8 * 64, 0xFFFFFFFF << 32, dtype=np.uint64)    # (padding cells of ragged maps: no node, no flags)
    words[tix.ravel()] = (flags.astype(np.uint64) | (num << np.uint64(32))).ravel()
    return words, int(node.sum())


def write_case(path, k, tag):
    maps = [k[f"{tag}_{n}"] for n in ("allowed_dirs_map", "is_road_map", "road_type_map", "intersection_map", "occupancy_map", "stop_map", "density32")]
    words, n_nodes = amap_words(*maps)
    H, W = maps[1].shape
    q = np.ascontiguousarray(k[f"{tag}_queries"], dtype=np.int64)
    q[:, 6] = np.minimum(q[:, 6], 0x7FFFFFFF)
    off, xy = k[f"{tag}_path_off"].astype(np.int32), np.ascontiguousarray(k[f"{tag}_path_xy"], dtype=np.int32).reshape(-1, 2)
    assert q.shape[1] == 7 and len(off) == len(q) + 1 and off[-1] == len(xy)
    head = np.array([0x48545341, W, H, n_nodes, LDS_HEAP + min(4 * W * H, 1 << 18), 1, 1, TURN2, CONTRA2, STOP2, *RT2, len(q), len(xy)], dtype=np.int32)
    with open(path, "wb") as f:
        for a in (head, words, q.astype(np.int32), off, xy):
            f.write(np.ascontiguousarray(a).tobytes())
    return len(q)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    k = np.load(os.path.join(GOLDEN, "astar_kats.npz"))
    d = tmp_path_factory.mktemp("astar_host")
    paths, n = [], 0
    for tag in ("a", "b"):
        p = str(d / f"case_{tag}.bin")
        n += write_case(p, k, tag)
        paths.append(p)
    assert n == 520
    return paths


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("asan", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
                                        ("tsan", ["-g", "-O1", "-fsanitize=thread"])])
def test_host_searcher_reproduces_the_reference_paths(cases, name, flags):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"astar_host_check_{name}")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC, *HDRS]):
        subprocess.run(["g++", "-std=c++17", "-pthread", *flags, "-I", INC, "-o", exe, SRC], check=True)
    p = subprocess.run([exe, *cases], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("astar host ok: 520 queries"), (p.stdout + p.stderr)[-2000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
