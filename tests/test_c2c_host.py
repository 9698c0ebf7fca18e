"""CPU checks of the cloud-to-cloud entries (lk_clouds_c2c_dev / lk_clouds_c2c): the case table of tests/c2ccases.py against its 50-digit values
through the numpy statement legkilo_amd.cloudmetrics.c2c, leg-kilo_amd/csrc/lk_c2c.h compiled for the host as a stand-alone program
(tools/probes/c2c_host.cc: the CPU twin of the device route - cells, clipping, floor, edge doubling) under the address and undefined-behaviour
sanitizers on every case, the same program with the clipping taken out, scipy's k-d tree where scipy imports, cloudmetrics.fscore, the C++ wrapper,
and the C-ABI: lk_c2c's size and field offsets from a C program compiled against the header, the exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import c2ccases as cc
from legkilo_amd import abi, binding, cloudmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "c2c_host.cc")
NEW_SYMBOLS = ["lk_clouds_c2c_dev", "lk_clouds_c2c"]
FIELDS = ["rmse", "mean", "max", "n_query", "n_matched", "n_within", "worst", "status"]


@pytest.fixture(scope="module")
def golden():
    return cc.golden()


@pytest.fixture(scope="module")
def brute():
    """cloudmetrics.c2c of every case, once."""
    return {n: cloudmetrics.c2c(c["query"], c["ref"], c["max_dist"], c["thr"]) for n, c in cc.CASES.items()}


def test_table_holds_what_the_issue_lists(golden):
    sizes = {s for pair in cc.SIZES for s in pair}
    assert sizes == {0, 1, 2, 63, 64, 65, 257} and (0, 65) in cc.SIZES and (65, 0) in cc.SIZES
    for nq, nr in cc.SIZES:
        c = cc.CASES[f"s{nq}_{nr}"]
        assert (len(c["query"]), len(c["ref"])) == (nq, nr)
    assert golden["s65_0"]["n_matched"] == 0 and np.isnan(golden["s65_0"]["rmse"]) and golden["s65_0"]["status"] == 0
    assert len(cc.DIRECTIONS) == 26
    for d in cc.DIRECTIONS:   # the one reference point in reach is record 2, and it lies in the neighbour cell the name says
        c, g = cc.CASES[cc.dir_name(d)], golden[cc.dir_name(d)]
        assert g["j"].tolist() == [2] and g["n_matched"] == 1
        cell = lambda p: np.floor(p.astype(np.float64) / c["max_dist"])   # noqa: E731
        assert tuple((cell(c["ref"][2]) - cell(c["query"][0])).astype(int)) == d
    for name in ("in_block_out_of_reach", "two_cells_away"):
        assert golden[name]["n_matched"] == 0 and golden[name]["j"].tolist() == [cc.NO_MATCH]
    for face in cc.FACES:
        assert golden[f"outside_{face}"]["matched"].tolist() == [True, False, False]
    assert golden["wrap_trap"]["j"].tolist() == [0]
    assert len(cc.CASES["heavy_cell"]["ref"]) == 5002 and golden["heavy_cell"]["n_matched"] >= 24
    z = cc.CASES["around_zero"]
    assert (np.abs(z["query"][:8]) < 1e-6).all() and (np.abs(z["ref"][-8:]) < 1e-6).all() and (z["ref"][-8:] < 0).any() and golden["around_zero"]["matched"][:8].all()
    assert golden["around_zero"]["j"][:8].tolist() == list(range(100, 108))
    assert golden["dup_ref"]["j"][:7].tolist() == [4, 3, 2, 1, 0, 4, 3]   # the copies that come first in the reversed cloud, not the originals behind them
    assert golden["exact_ties"]["j"].tolist() == [0, 5]
    assert golden["reach_exact"]["matched"].tolist() == [True, False, True] and golden["reach_exact"]["n_within"].tolist() == [1, 2]
    assert golden["reach_exact"]["max"] == cc.CASES["reach_exact"]["max_dist"] == 5 * 2.0 ** -4
    f = cc.CASES["far_clusters"]
    assert f["max_dist"] == 0.05 and np.linalg.norm(f["ref"][64:].mean(0) - f["ref"][:64].mean(0)) > 2900 and golden["far_clusters"]["n_matched"] >= 2
    assert cc.CASES["one_cell"]["max_dist"] > np.ptp(cc.CASES["one_cell"]["ref"], axis=0).max() and golden["one_cell"]["n_matched"] == 30
    s = golden["self"]
    assert [s[k] for k in ("rmse", "mean", "max")] == [0.0, 0.0, 0.0] and s["n_matched"] == 96 and s["worst"] == 0
    want = np.arange(96)
    want[[40, 41, 90]] = 7
    assert s["j"].tolist() == want.tolist()
    for name, st in (("nan_query", 1), ("inf_query", 1), ("nan_ref", 1), ("inf_ref", 1), ("range_query", 2), ("range_ref", 2), ("range_edge_inside", 0)):
        assert golden[name]["status"] == st and (golden[name]["n_matched"] == 0) == bool(st), name
    assert cc.C == 16.0 * max(1.0, cc.NUMPY_RATIO) and os.path.getsize(cc.GOLDEN) < 500 << 10


def load_generator():
    spec = importlib.util.spec_from_file_location("make_c2c_cases", os.path.join(ROOT, "tests", "golden", "make_c2c_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_file_regenerates_to_the_bit():
    mod = load_generator()
    again = mod.evaluate(cc.CASES)   # (from the frozen inputs; the generator's 50-digit assertions run again)
    again.update(mod.inputs(cc.CASES))
    z = np.load(cc.GOLDEN)
    assert sorted(again) == sorted(z.files)
    for k in z.files:
        assert again[k].dtype == z[k].dtype and again[k].shape == z[k].shape and again[k].tobytes() == z[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    fresh = cc.build()
    assert list(fresh) == cc.NAMES
    for name, c in fresh.items():
        f = cc.CASES[name]
        assert c["max_dist"] == f["max_dist"] and np.array_equal(c["thr"], f["thr"]), name
        for k in ("query", "ref"):
            assert c[k].shape == f[k].shape and np.array_equal(np.isnan(c[k]), np.isnan(f[k])), (name, k)
            fin = np.isfinite(f[k])
            assert np.array_equal(c[k][~fin], f[k][~fin], equal_nan=True) and np.allclose(c[k][fin], f[k][fin], rtol=1e-6, atol=1e-12), (name, k)


def test_numpy_statement_is_exact_on_decisions_and_within_c_on_figures(golden, brute):
    worst = (0.0, None)
    for name, c in cc.CASES.items():
        got, want = brute[name], golden[name]
        assert np.array_equal(got["j"], want["j"]) and np.array_equal(got["matched"], want["matched"]), name
        assert (got["n_query"], got["n_matched"], got["worst"], got["status"]) == (len(c["query"]), want["n_matched"], want["worst"], want["status"]), name
        assert list(got["n_within"]) == want["n_within"].tolist(), name
        assert np.isinf(got["d2"][~want["matched"]]).all() and (got["j"][~want["matched"]] == cc.NO_MATCH).all(), name
        for f in ("rmse", "mean", "max"):
            assert np.isnan(got[f]) == np.isnan(want[f]), (name, f)
            if not np.isnan(want[f]):
                ratio = abs(got[f] - want[f]) / (cc.ULP * c["max_dist"])
                assert ratio <= cc.C, (name, f, ratio)
                if ratio > worst[0]:
                    worst = (ratio, (name, f))
    print(f"cloudmetrics.c2c against the 50-digit figures: worst ratio {worst[0]:.3f} at {worst[1]} (NUMPY_RATIO {cc.NUMPY_RATIO})")
    assert worst[0] <= 2.0 * cc.NUMPY_RATIO
    assert all(v == 0.0 for v in brute["self"]["d2"]) and brute["self"]["rmse"] == 0.0


def build_probe(tmp, *flags):
    exe = tmp / ("c2c_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *flags, "-o", str(exe), PROBE], check=True, capture_output=True, text=True)
    return exe


def run_probe(exe, tmp, names):
    """The probe over the named cases -> {name: dict(header fields, j, d2, seen)}."""
    path = tmp / "pairs.bin"
    with open(path, "wb") as f:
        for n in names:
            c = cc.CASES[n]
            f.write(np.float64(c["max_dist"]).tobytes() + np.array([len(c["query"]), len(c["ref"])], dtype=np.uint64).tobytes())
            f.write(c["query"].tobytes() + c["ref"].tobytes())
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), {}, 0
    for n in names:
        h = lines[at].split()
        assert h[0] == "pair" and int(h[1]) == len(cc.CASES[n]["query"]), lines[at]
        nq = int(h[1])
        rows = [ln.split() for ln in lines[at + 1:at + 1 + nq]]
        out[n] = dict(status=int(h[4]), edge=float.fromhex(h[6]), doublings=int(h[8]), cells=[int(v) for v in h[10:13]],
                      j=np.array([int(r[0]) for r in rows], dtype=np.uint32), d2=np.array([float.fromhex(r[1]) for r in rows], dtype=np.float64),
                      seen=np.array([int(r[2]) for r in rows], dtype=np.int64))
        at += 1 + nq
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("c2c_probe")
    return tmp, build_probe(tmp)


def test_grid_search_on_the_host_under_sanitizers(golden, brute, probe):
    """lk_c2c.h's grid search on every case: clean under the sanitizers, (j, d2) equal to the brute force bit for bit - the clipping at the
    reference's faces, floor for negative coordinates and the doubled edge are checked here on the CPU."""
    tmp, exe = probe
    got = run_probe(exe, tmp, cc.NAMES)
    for name, c in cc.CASES.items():
        g, b = got[name], brute[name]
        assert g["status"] == golden[name]["status"], name
        assert np.array_equal(g["j"], b["j"]) and g["d2"].tobytes() == b["d2"].tobytes(), name
        assert np.array_equal(g["j"], golden[name]["j"]), name
    far, one = got["far_clusters"], got["one_cell"]
    assert far["doublings"] >= 1 and far["edge"] == 0.05 * 2.0 ** far["doublings"] and np.prod(np.array(far["cells"], dtype=np.float64)) < 2.0 ** 31
    r64 = cc.CASES["far_clusters"]["ref"].astype(np.float64)
    cells = lambda edge: np.floor(r64.max(0) / edge) - np.floor(r64.min(0) / edge) + 1   # noqa: E731
    assert cells(far["edge"]).tolist() == far["cells"] and np.prod(cells(far["edge"] / 2)) >= 2.0 ** 31   # ... and not once more than it had to
    assert one["cells"] == [1, 1, 1] and one["doublings"] == 0 and (one["seen"] == 50).all()
    assert got["range_edge_inside"]["cells"][0] == 2 ** 30 - 63 and got["range_edge_inside"]["doublings"] == 0
    assert got["wrap_trap"]["cells"] == [6, 2, 1] and got["wrap_trap"]["seen"].tolist() == [1]    # A alone: B, first cell of the next row, is not looked at
    assert got["two_cells_away"]["seen"].tolist() == [0] and got["in_block_out_of_reach"]["seen"].tolist() == [1]
    assert (got["heavy_cell"]["seen"][:24] >= 5000).all() and got["heavy_cell"]["seen"][-1] == 0
    bad = subprocess.run([str(exe), str(tmp / "missing.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "cannot open" in bad.stderr
    (tmp / "short.bin").write_bytes(np.float64(0.25).tobytes() + np.array([3, 0], dtype=np.uint64).tobytes() + b"\0" * 8)
    bad = subprocess.run([str(exe), str(tmp / "short.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "truncated" in bad.stderr


def test_without_the_clip_the_wrap_case_fails(probe):
    """-DLK_C2C_WRAP_BUG: a row's x range as plain i - 1 .. i + 1.  The query beyond x-max then looks at the first cell of the NEXT row.  The
    distance test still rejects what lies there, so (j, d2) stand; what fails is the check of the records looked at."""
    tmp, _ = probe
    got = run_probe(build_probe(tmp, "-DLK_C2C_WRAP_BUG"), tmp, ["wrap_trap"])["wrap_trap"]
    assert got["seen"].tolist() == [2] and got["seen"].tolist() != [1]
    assert got["j"].tolist() == [0]


def test_kd_tree_agrees_where_the_runner_up_is_separated(golden):
    spatial = pytest.importorskip("scipy.spatial")
    n = 0
    for name, c in cc.CASES.items():
        g = golden[name]
        if g["status"] or not len(c["ref"]) or not len(c["query"]):
            continue
        r64, q64 = c["ref"].astype(np.float64), c["query"].astype(np.float64)
        d, j = spatial.cKDTree(r64).query(q64, k=min(2, len(r64)))
        d, j = d.reshape(len(q64), -1), j.reshape(len(q64), -1)
        sep = g["matched"] & ((d[:, -1] > d[:, 0] * (1 + 1e-9)) if d.shape[1] > 1 else True)
        assert np.array_equal(j[sep, 0], g["j"][sep]), name
        assert np.array_equal(d[:, 0] <= c["max_dist"] * (1 - 1e-9), g["matched"]) or name == "reach_exact", name
        n += int(sep.sum())
    assert n > 500


def test_fscore_arithmetic():
    rec = np.zeros(2, dtype=abi.c2c_dtype())
    rec["n_query"], rec["n_within"] = [200, 50], [[100, 150, 0, 0], [40, 50, 0, 0]]
    assert cloudmetrics.fscore(rec[0], rec[1], 0) == (0.5, 0.8, 2 * 0.5 * 0.8 / 1.3)
    assert cloudmetrics.fscore(rec[0], rec[1], 1) == (0.75, 1.0, 2 * 0.75 / 1.75)
    assert cloudmetrics.fscore(rec[0], rec[1], 2) == (0.0, 0.0, 0.0)
    empty = dict(n_query=0, n_within=[0])
    assert cloudmetrics.fscore(empty, dict(n_query=4, n_within=[2]), 0) == (0.0, 0.5, 0.0)
    a = cloudmetrics.c2c(cc.CASES["s64_65"]["query"], cc.CASES["s64_65"]["ref"], cc.M, cc.THR)
    b = cloudmetrics.c2c(cc.CASES["s64_65"]["ref"], cc.CASES["s64_65"]["query"], cc.M, cc.THR)
    p, r, f = cloudmetrics.fscore(a, b, 2)
    assert (p, r) == (a["n_matched"] / 64, b["n_matched"] / 65) and f == pytest.approx(2 * p * r / (p + r))


def test_c2c_record_is_80_bytes():
    assert C.sizeof(abi.lk_c2c) == 80 and abi.c2c_dtype().itemsize == 80
    assert [f for f, _ in abi.lk_c2c._fields_] == FIELDS == list(abi.c2c_dtype().names)
    assert (abi.LK_C2C_NONFINITE, abi.LK_C2C_RANGE) == (cloudmetrics.LK_C2C_NONFINITE, cloudmetrics.LK_C2C_RANGE) and abi.LK_C2C_NO_MATCH == cloudmetrics.NO_MATCH


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + " %u %u\\n\", sizeof(lk_c2c), "
                   + ", ".join(f"offsetof(lk_c2c, {f})" for f in FIELDS) + ", LK_C2C_NONFINITE, LK_C2C_RANGE); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 80
    assert got[1:9] == [getattr(abi.lk_c2c, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 72, 76]
    assert got[1:9] == [abi.c2c_dtype().fields[f][1] for f in FIELDS]
    assert got[9:11] == [abi.LK_C2C_NONFINITE, abi.LK_C2C_RANGE] == [1, 2]


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS and s in sigs and len(sigs[s][1]) == 17
        assert sigs[s][1][10:13] == [C.c_double, C.c_void_p, C.c_uint32]
    assert callable(binding.LegKiloHip.clouds_c2c_dev) and callable(binding.LegKiloHip.clouds_c2c)
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for phrase in ("d2 = (dx*dx + dy*dy) + dz*dz", "the smallest index on equal d2", "d2_i <= max_dist * max_dist", "0xffffffff and +inf", "LK_C2C_RANGE"):
        assert phrase in hdr, phrase   # the definition the tests implement stands in the header


def test_host_header_compiles_with_the_new_wrapper(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::cloudsC2cDev;\nint main() { return a ? 0 : 1; }\n')
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
