"""CPU test of the GEMM launch planner on its own (clipcap_amd/csrc/gemm_plan.h): tests/gemm_plan_check.cpp includes only that header and is
compiled with the host compiler and no HIP include path — which is the proof that the header is HIP-free —, plainly and with
-fsanitize=address,undefined, and run directly.  It checks the K-slice function over K in 64..8192 and 1..9 slices and the rows of
DESIGN.md 4.1's tile table that state a choice."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_planner_alone(tmp_path, sanitize):
    assert CXX, "no host C++ compiler"
    exe = str(tmp_path / "gemm_plan_check")
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-I", os.path.join(ROOT, "clipcap_amd", "csrc")]
    # (the sanitizer runtimes linked statically: the program does not depend on the order in which shared libraries are loaded)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(CXX) and "clang" not in os.path.basename(CXX) else ["-static-libsan"]
    flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static] if sanitize else []
    subprocess.run([CXX, *flags, os.path.join(ROOT, "tests", "gemm_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("ok:")
