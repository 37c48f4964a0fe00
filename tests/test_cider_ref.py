"""CPU tests of the CIDEr-D statement: tests/cider_ref.py (float64, dicts) against the scores the reference project's CiderScorer gave on
the recorded cases (tests/golden/cider_ref.npz, written by tools/gen_cider_golden.py), and clipcap_amd/csrc/cider_table.h on its own —
tests/cider_table_check.cpp includes only that header and is compiled with the host compiler and no HIP include path, plainly and with
-fsanitize=address,undefined, and run directly."""
import os
import shutil
import subprocess

import pytest

from tests import cider_ref
from tests.cider_cases import golden_cases, pack, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def test_statement_reproduces_the_reference_scorer():
    """idf from the reference scorer's own document frequencies, N = the images of the case: within 1e-12 of its scores (they are <= 10)."""
    cases = golden_cases()
    assert len(cases) >= 20
    worst, n, zeros, short = 0.0, 0, 0, 0
    for case in cases:
        idf = cider_ref.idf_from_df(case["df"], len(case["images"]))
        for (cand, refs), want in zip(case["images"], case["score"]):
            got = cider_ref.cider_d(cand, refs, idf)
            worst = max(worst, abs(got - want))
            n += 1
            zeros += want == 0.0
            short += len(cand) <= 1
    print(f"{n} candidates, {zeros} score 0, {short} of 0 or 1 words; largest difference {worst:.3e}")
    assert n >= 80 and short >= 3 and zeros < n // 2
    assert worst <= 1e-12


def test_own_document_frequencies_equal_the_reference_scorers():
    for case in golden_cases():
        assert dict(cider_ref.doc_freq([refs for _, refs in case["images"]])) == case["df"]


def test_key_helpers_round_trip():
    for g in [(0,), (0, 0), (65534,), (1, 2, 3), (40, 0, 40, 0), (65534, 65534, 65534, 65534)]:
        assert unpack(pack(g)) == g
    assert pack((0,)) == 0xFFFFFFFFFFFF0000 and pack((1, 2, 3, 4)) == 0x0004000300020001


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_table_header_alone(tmp_path, sanitize):
    assert CXX, "no host C++ compiler"
    exe = str(tmp_path / "cider_table_check")
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-I", os.path.join(ROOT, "clipcap_amd", "csrc")]
    # (the sanitizer runtimes linked statically: the program does not depend on the order in which shared libraries are loaded)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(CXX) and "clang" not in os.path.basename(CXX) else ["-static-libsan"]
    flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static] if sanitize else []
    subprocess.run([CXX, *flags, os.path.join(ROOT, "tests", "cider_table_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("ok:")
