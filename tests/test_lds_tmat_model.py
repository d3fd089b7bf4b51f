"""csrc/tspgpu_lds_tmat.h -- the index arithmetic of the tour-ordered matrix copy that the TM instantiations of k_lds2opt
fetch moved rows from -- and the protocol around it, on the CPU (tests/lds_tmat_main.cpp).  A stand-alone program built with
AddressSanitizer and UBSan and run as a child process.  Arithmetic: a row assembled chunk by chunk from the row before a
move equals the row with the range reversed (n = 16 and 64 exhaustively, n = 1024 sampled over every lo mod 8, M mod 8 and
ranges across the array end), at most 3 chunks of a row go cell by cell, the write-back chunks cover every changed cell.
Protocol: W workgroups of E + 1 rows, thousands of random moves in three workgroup orders; behind every move tmat and every
LDS row equal the truth, and a row of tmat has one writer and at most one reader, the same workgroup.  Fetching the copy
row from tmat as well must be caught.  CPU only."""
import os
import subprocess

import pytest

# the compiler flags and the skip rule are test_mem_owner's, as in test_relaunch_protocol
from test_mem_owner import CSRC, ROOT, SAN, asan_links


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lds_tmat")
    if not asan_links(tmp):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    out = str(tmp / "lds_tmat")
    r = subprocess.run(["g++", *SAN, "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", out, os.path.join(ROOT, "tests", "lds_tmat_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_arithmetic_and_protocol(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "lds_tmat ok"


def test_copy_row_fetched_from_tmat_is_caught(exe):
    """the one row with two fetchers: its owner rewrites tmat[x] in the sweep in which the neighbour would read it"""
    r = subprocess.run([exe, "--no-copy-rule"], capture_output=True, text=True)
    assert r.returncode == 3, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("violation:")
