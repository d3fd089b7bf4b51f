"""csrc/tspgpu_looks.h -- the loop that m2_run, or_run, or_descent_batch, nlb_descent and nlv_walks share: rounds of launches,
then a look at the control block(s) -- over scripted rounds and looks and a fake clock (tests/looks_main.cpp).  A stand-alone
program built with AddressSanitizer and UBSan and run as a child process.  With launch and look counts compared exactly:
per_look rounds between looks without a deadline (4 and 8), one under a deadline, nothing at all behind a deadline already
passed, a deadline passing between groups, an error from the k-th round of a group (no look behind it) and from a look, a
stop at the first look; and for the live list its order, the entries the predicate drops, uploads only on a shrink to a
non-empty list, the end on empty, the largest length, the per-group hook and an empty list on entry.  CPU only."""
import os
import subprocess

import pytest

# the compiler flags and the skip rule are test_mem_owner's, as in test_relaunch_protocol
from test_mem_owner import CSRC, ROOT, SAN, asan_links


def test_look_loop_over_scripted_rounds_and_looks(tmp_path):
    if not asan_links(tmp_path):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp_path / "looks")
    r = subprocess.run(["g++", *SAN, "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "looks_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "looks ok"
