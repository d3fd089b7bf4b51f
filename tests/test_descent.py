"""csrc/tspgpu_descent.h -- the descent over the neighbour lists on one tour: { 2-opt; Or-opt } until an Or-opt phase applies
nothing, then a 3-opt phase where the descent has one, all of it until a 3-opt phase applies nothing -- against transcriptions
of the three loops it replaced (ornl_descent, nl3_descent with its nested call, dl_descent) over a scripted phase function
(tests/descent_main.cpp).  A stand-alone program built with AddressSanitizer and UBSan and run as a child process.  Compared
field by field -- the code, every counter, the peaks of max_k, late, the looked totals, the ordered list of phases asked
for -- with and without a 3-opt phase, plain against ornl_descent / nl3_descent and with looks against dl_descent: every
pattern of moves in {0, > 0} over three outer rounds of three inner rounds, and behind each of them the k-th phase ending
late and the k-th phase answering a code, for every k.  CPU only."""
import os
import subprocess

import pytest

# the compiler flags and the skip rule are test_mem_owner's, as in test_looks
from test_mem_owner import CSRC, ROOT, SAN, asan_links


def test_descent_against_the_loops_it_replaced(tmp_path):
    if not asan_links(tmp_path):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp_path / "descent")
    r = subprocess.run(["g++", *SAN, "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "descent_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "descent ok"
