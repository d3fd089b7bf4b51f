"""csrc/tspgpu_relaunch.h -- the protocol that run_persist and run_pstream follow around the one-launch kernels -- over a
scripted launch and a fake clock (tests/relaunch_main.cpp).  A stand-alone program built with AddressSanitizer and UBSan
and run as a child process: the gate (skip, back-off 16, 32 .. 1024, "never", the reset after a launch that came up), the
sweep budget of every launch against the formula recomputed from the script, a refused launch, a failed rendezvous on the
first and on a later launch, the retries counted over the whole descent, a lost exchange, a status that was never
written, and the family's `completed` and `lost` callables deciding.  No launch fails on any GPU for it.  CPU only."""
import os
import subprocess

import pytest

# the compiler flags and the skip rule are test_mem_owner's, on purpose the same ones; this module therefore needs that
# one beside it (tests/ is on sys.path: rootdir conftest) -- rename or remove it and these four names move here
from test_mem_owner import CSRC, ROOT, SAN, asan_links


def test_relaunch_protocol_over_a_scripted_launch(tmp_path):
    if not asan_links(tmp_path):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp_path / "relaunch")
    r = subprocess.run(["g++", *SAN, "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "relaunch_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "relaunch ok"
