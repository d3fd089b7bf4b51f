"""csrc/tspgpu_plan.h -- where the 2-opt launch plans are decided: the per-sweep plan (plan::decide), the forms of the
LDS-resident descent (plan::resident), the streamed descent (plan::stream), the matrix-free kernel (plan::otf8, otf_early) and
the candidate sweeps' geometry (plan::sweep_geom) -- over the case table of tests/golden/golden_plan.json
(tests/plan_main.cpp).  A stand-alone program built with AddressSanitizer and UBSan and run as a child process; CPU only.

The golden's *_out rows were recorded from the logic of the commit its header names, before that logic moved into the
header: every field of every case must be equal, so no plan moves unnoticed.  The anchors are figures that the code's own
comments state, and the contract of the one caller: a refused plan replaces nothing."""
import json
import os
import subprocess

import pytest

# the compiler flags and the skip rule are test_mem_owner's, as in test_relaunch_protocol
from test_mem_owner import CSRC, ROOT, SAN, asan_links

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_plan.json")
SECTIONS = ("sweep", "option", "otf", "resident", "stream", "none", "geom")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan")
    if not asan_links(tmp):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp / "plan")
    r = subprocess.run(["g++", *SAN, "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "plan_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_decision_of_the_table_is_the_recorded_one(program, golden):
    r = subprocess.run([program, GOLDEN], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = {s: [] for s in SECTIONS}
    for line in r.stdout.splitlines():
        what, *values = line.split()
        got[what].append([int(v) for v in values])
    for s in SECTIONS:
        want = golden[s + "_out"]
        assert len(got[s]) == len(want) > 0, (s, len(got[s]), len(want))
        differ = [(i, g, w) for i, (g, w) in enumerate(zip(got[s], want)) if g != w]
        assert not differ, (s, len(differ), differ[:5])


def test_the_table_reaches_every_refusal_and_every_form(golden):
    """so that the table cannot lose them silently: the five refusals of plan::decide (column 0 of a sweep row), every kernel,
    the three answers of plan::resident, both answers of plan::stream, and "none" for what the one-launch descents do not take"""
    rows = golden["sweep_out"] + golden["option_out"]
    assert {r[0] for r in rows} == {0, 1, 2, 3, 4, 5}, sorted({r[0] for r in rows})
    assert {r[1] for r in rows if r[0] == 0} == {1, 2, 3}
    assert {r[3] for r in golden["otf_out"]} == {4} and {tuple(r[:2]) for r in golden["otf_out"]} == {(0, 0), (1, 0), (1, 1)}
    assert {r[0] for r in golden["resident_out"]} == {0, 1, 2}
    assert {r[6] for r in golden["resident_out"]} == {0, 1}
    assert {r[0] for r in golden["stream_out"]} == {0, 1}
    assert golden["none_out"] and all(r == [0, 0, 0, 0, 0, 0, 1] + [0] * 6 for r in golden["none_out"]), golden["none_out"]
    # the axes the table is built over
    assert golden["devices"] == [[256, 163840], [64, 65536], [304, 65536]] and golden["elems"] == [3, 2, 1]
    assert golden["ns"] == [5, 8, 63, 64, 255, 256, 1000, 1024, 2048, 4095, 4096, 4097, 4461, 5400, 6144, 8191, 8192, 12288, 16383, 16384, 18512,
                            33810, 65536, 65537]
    assert golden["ntours"] == [1, 2, 4, 5, 64, 256] and golden["occ"][:4] == [0, 1, 2, 8]


def test_anchors_and_a_refusal_replaces_nothing(program):
    r = subprocess.run([program, "anchors"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "anchors ok"
