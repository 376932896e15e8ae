"""The formats the A* searchers share (csrc/astar_words.h) on the CPU: tests/native/astar_words_check.cpp round-trips the snapshot
word through its accessors for every combination of the flag bits, checks the tiled index against its formula on a ragged map,
k_replan's table record against its epoch, and the penalties in half units against the constants tests/test_host_astar_native.py
carries - under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain executable."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "astar_words_check.cpp")
INC = os.path.join(HERE, "..", "trafficsimulation_amd", "csrc")
HDRS = [os.path.join(INC, h) for h in ("astar_words.h", "arena_epochs.h", "path_words.h")]
BUILD = os.path.join(HERE, "native", "_build")


def test_snapshot_word_tiled_index_table_record_and_half_costs():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "astar_words_asan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC, *HDRS]):
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INC,
                        "-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("astar words ok"), (p.stdout + p.stderr)[-2000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
