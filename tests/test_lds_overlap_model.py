"""The biased packed deltas of the shaped row loop of k_lds2opt on the CPU (tests/lds_overlap_main.cpp over
csrc/tspgpu_lds_tmat.h: pk_bias, pk_biased, PK_BIAS).  A stand-alone program built with AddressSanitizer and UBSan and run
as a child process: over x, y, w[k], w[m] in {0, 1, 2, 8190, 16382, 16383}^4 (both halves, and the halves at opposite ends)
and a million draws in [0, 16383] the biased unsigned halves XOR 0x8000 are the signed deltas of the unbiased form, the
32-bit sum has no carry between its halves, every half stays in the range the kernel's comment states, and the unsigned
order of the biased halves is the signed order of the deltas.  CPU only."""
import os
import subprocess

import pytest

# the compiler flags and the skip rule are test_mem_owner's, as in test_lds_tmat_model
from test_mem_owner import CSRC, ROOT, SAN, asan_links


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lds_overlap")
    if not asan_links(tmp):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    out = str(tmp / "lds_overlap")
    r = subprocess.run(["g++", *SAN, "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", out, os.path.join(ROOT, "tests", "lds_overlap_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_bias_arithmetic(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "lds_overlap ok"
