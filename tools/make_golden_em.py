"""Writes tests/golden/golden_extra_mileage.json: Extra Mileage (h_ExtraMileage, EM_MAX) on the 14 instances of the
reference's published heuristics table -- the farthest pair, then the reference's OWN h_extramileage_util called
through ctypes in oracle/_ref/libtspref.so (built by `make -C oracle`) -- with the cost, which must equal the published
ExtraMileage column, and the fnv1a hash of the successor array; plus fnl4461 from the incremental model of
tests/test_extra_mileage.py (the reference's O(n^3) loop takes minutes there).  The cost matrices are the reference's
own (tsp_compute_costs).

    python tools/make_golden_em.py            # the 14 published instances + fnl4461 (rewrites the file)
    python tools/make_golden_em.py --large    # adds d18512 (EUC_2D) and pla85900 (CEIL_2D) from tools/em_model.c, the
                                              # C restatement, after checking it against the reference's records
"""
import ctypes as C
import importlib.util
import subprocess
import tempfile
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libtspref.so")
DATA = os.path.join(ROOT, "tests", "golden", "data")


class Sol(C.Structure):        # tsp_solution, utils.h:42-47
    _fields_ = [("cost", C.c_double), ("path", C.POINTER(C.c_int)), ("ncomp", C.c_int), ("comp", C.POINTER(C.c_int))]


def fnv1a(succ):
    h = 0xcbf29ce484222325                                  # one 32-bit word per node, as the tests hash
    for x in np.asarray(succ, np.int64):
        h = ((h ^ (int(x) & 0xFFFFFFFF)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def model():
    spec = importlib.util.spec_from_file_location("tem", os.path.join(ROOT, "tests", "test_extra_mileage.py"))
    tem = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tem)
    return tem


# results/heuristics-ric.csv of the reference, column ExtraMileage
PUBLISHED = {"rl1304": 307898, "pr1002": 302240, "vm1748": 403144, "rl1323": 329371, "u1060": 267431, "rl1889": 386958,
             "vm1084": 274081, "u1817": 66988, "nrw1379": 65291, "pcb1173": 69984, "fl1577": 26944, "fl1400": 22532,
             "d1291": 59918, "d1655": 73473}


def main():
    L = C.CDLL(REF_SO)
    L.refdrv_init.argtypes = [C.c_char_p]
    L.refdrv_read_file.argtypes = [C.c_char_p]
    L.refdrv_costs.restype = C.POINTER(C.c_double)
    L.h_extramileage_util.argtypes = [C.POINTER(Sol), C.c_int, C.c_int]
    L.h_extramileage_util.restype = C.c_int
    L.refdrv_init(os.path.join(ROOT, "oracle", "_ref", "scratch").encode())
    tem = model()

    def costs(name):
        L.refdrv_read_file(os.path.join(DATA, name + ".tsp").encode())
        n = L.refdrv_n()
        return np.ctypeslib.as_array(L.refdrv_costs(), shape=(n, n)).copy()

    out = {"_generator": "tools/make_golden_em.py", "_source": "results/heuristics-ric.csv (column ExtraMileage)",
           "published": {}, "extra": {}}
    for name in sorted(PUBLISHED):
        c = costs(name)
        n = len(c)
        a, b = tem.farthest_pair(c)
        path = np.zeros(n, dtype=np.int32)
        path[a], path[b] = b, a
        s = Sol(2.0 * c[a, b], path.ctypes.data_as(C.POINTER(C.c_int)), 0, None)
        t = time.time()
        assert L.h_extramileage_util(C.byref(s), a, b) == 0
        assert sorted(path) == list(range(n))
        out["published"][name] = {"n": n, "a": a, "b": b, "cost": s.cost, "published": float(PUBLISHED[name]),
                                  "fnv": "%016x" % fnv1a(path)}
        print(name, a, b, s.cost, PUBLISHED[name], "%.1fs" % (time.time() - t), flush=True)
        assert s.cost == PUBLISHED[name], name
    c = costs("fnl4461")
    a, b = tem.farthest_pair(c)
    succ, cost, stale = tem.em_model(c, a, b)
    out["extra"]["fnl4461"] = {"n": len(c), "a": a, "b": b, "cost": cost, "fnv": "%016x" % fnv1a(succ), "stale": stale,
                               "source": "incremental model"}
    print("fnl4461", a, b, cost, stale, flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "golden_extra_mileage.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def run_c_model(exe, xy, kind, tmp):
    path = os.path.join(tmp, "xy.bin")
    np.ascontiguousarray(xy, np.float64).tofile(path)
    a, b, cost, fnv, stale = subprocess.run([exe, path, str(len(xy)), str(kind)], check=True, capture_output=True,
                                            text=True).stdout.split()
    return int(a), int(b), float(cost), fnv, int(stale)


def large():
    from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib   # (the product's TSPLIB reader)
    gpath = os.path.join(ROOT, "tests", "golden", "golden_extra_mileage.json")
    with open(gpath) as f:
        out = json.load(f)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "em_model")
        subprocess.run(["gcc", "-O3", "-fopenmp", "-ffp-contract=off", "-fno-math-errno", "-o", exe,
                        os.path.join(ROOT, "tools", "em_model.c"), "-lm"], check=True)
        # the C restatement first reproduces every record the reference made
        for name, rec in sorted(out["published"].items()):
            xy, kind = read_tsplib(os.path.join(DATA, name + ".tsp"))
            got = run_c_model(exe, xy, kind, tmp)
            assert got[:4] == (rec["a"], rec["b"], rec["cost"], rec["fnv"]), (name, got, rec)
        for name in ["d18512", "pla85900"]:
            xy, kind = read_tsplib(os.path.join(DATA, name + ".tsp"))
            t = time.time()
            a, b, cost, fnv, stale = run_c_model(exe, xy, kind, tmp)
            out["extra"][name] = {"n": len(xy), "kind": int(kind), "a": a, "b": b, "cost": cost, "fnv": fnv, "stale": stale,
                                  "source": "tools/em_model.c (incremental model, C)"}
            print(name, a, b, cost, fnv, stale, "%.1fs" % (time.time() - t), flush=True)
    with open(gpath, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--large" in sys.argv:
        sys.path.insert(0, ROOT)
        large()
    else:
        main()
