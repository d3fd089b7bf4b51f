"""csrc/tspgpu_mem.h -- the owners of device and pinned memory and the two all-or-none routines -- over a fake backend
(tests/mem_owner_main.cpp: malloc, a table of live blocks, "fail the k-th allocation from now").  A stand-alone program
built with AddressSanitizer and UBSan and run as a child process: for every k up to the allocations of an operation,
and once without a failure, a buffer's alloc / reserve / move-assignment, alloc_all over three buffers, and the growth of
a four-row view from 2 to 5 units.  After a failure the view, its unit count, the old bytes and the live blocks are
as before; after success the kept rows begin with the old bytes and go on with the fill.  Exit status 0 also means that
LeakSanitizer found nothing left allocated.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "travellingsalesmanoptimization_amd", "csrc")
# -static-libasan: the sanitizer's runtime is linked into the program, so that it does not depend on library load order
SAN = ["-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]


def asan_links(tmp_path):
    """an empty program links with -fsanitize=address, runtime as in SAN (the one reason this test may skip)"""
    if not shutil.which("g++"):
        return False
    src = tmp_path / "empty.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address", "-static-libasan", "-o", str(tmp_path / "empty"), str(src)], capture_output=True, text=True)
    return r.returncode == 0


def test_owners_and_growth_under_injected_failures(tmp_path):
    if not asan_links(tmp_path):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp_path / "mem_owner")
    r = subprocess.run(["g++", *SAN, "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "mem_owner_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "mem_owner ok"
