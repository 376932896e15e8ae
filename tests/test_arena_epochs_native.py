"""The epoch ranges of k_replan's and the quads' table records (csrc/arena_epochs.h) on the CPU: tests/native/arena_epochs_test.cpp
walks every top byte of a 32-bit word against every epoch of both kernels - no record of one is live for the other, zero is live
for neither, the stamps wrap inside their ranges - and runs under AddressSanitizer and UndefinedBehaviorSanitizer as a plain
executable."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "arena_epochs_test.cpp")
INC = os.path.join(HERE, "..", "trafficsimulation_amd", "csrc")
HDR = os.path.join(INC, "arena_epochs.h")
BUILD = os.path.join(HERE, "native", "_build")


def test_no_record_of_one_kernel_is_live_for_the_other():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "arena_epochs_asan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INC,
                        "-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("arena epochs ok"), (p.stdout + p.stderr)[-2000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
