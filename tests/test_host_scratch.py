"""The scoped type for a call's temporary device buffers (csrc/scratch.h) on the CPU: tests/native/scratch_check.cpp stands in
for the five HIP names the header uses, refuses each allocation of a scope in turn, and runs under AddressSanitizer and
UndefinedBehaviorSanitizer as a plain executable."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "scratch_check.cpp")
HDR = os.path.join(HERE, "..", "trafficsimulation_amd", "csrc", "scratch.h")
BUILD = os.path.join(HERE, "native", "_build")


def test_scratch_frees_everything_on_every_way_out():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "scratch_check_asan")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok scratch"), (p.stdout + p.stderr)[-2000:]
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
