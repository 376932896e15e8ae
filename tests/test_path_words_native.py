"""The format of the vehicle paths in the pool (csrc/path_words.h) on the CPU: tests/native/path_words_check.cpp encodes strings of
0 to 100 steps from cells and from direction bytes, decodes and walks them, compares the two-word window with the single-step
reader on buffers of exactly the string's words, and the live-word rule of collections and checkpoints with a brute-force copy -
under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain executable."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "path_words_check.cpp")
INC = os.path.join(HERE, "..", "trafficsimulation_amd", "csrc")
HDRS = [os.path.join(INC, "path_words.h")]
BUILD = os.path.join(HERE, "native", "_build")


def test_encode_decode_walk_window_and_live_words():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "path_words_asan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC, *HDRS]):
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INC,
                        "-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("path words ok"), (p.stdout + p.stderr)[-2000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
