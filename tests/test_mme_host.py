"""CPU checks of the reference-free map scores (lk_clouds_mme_dev / lk_clouds_mme): the case table of tests/mmecases.py against its exact / 50-digit
values through the numpy statement legkilo_amd.cloudmetrics.mme, leg-kilo_amd/csrc/lk_mme.h compiled for the host as a stand-alone program
(tools/probes/mme_host.cc: the CPU twin of the device route - bounds, edge rule, keys, stable sort, walk, finish, the record's tree) under the address
and undefined-behaviour sanitizers on every case, the same program with truncation in the place of floor, wrong variants of the restatement that
each fail on a named case, scipy's k-d tree where scipy imports, the C++ wrapper, and the C-ABI: lk_mme's size and field offsets from a C program
compiled against the header, the exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import mmecases as mc
from legkilo_amd import abi, binding, cloudmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "mme_host.cc")
NEW_SYMBOLS = ["lk_clouds_mme_dev", "lk_clouds_mme"]
FIELDS = ["mme", "mpv", "h_max", "n_points", "n_dense", "n_scored", "n_pairs", "worst", "status"]


@pytest.fixture(scope="module")
def golden():
    return mc.golden()


@pytest.fixture(scope="module")
def brute():
    """cloudmetrics.mme of every case, once."""
    return {n: cloudmetrics.mme(c["cloud"], c["radius"], c["min_pts"]) for n, c in mc.CASES.items()}


def load_generator():
    spec = importlib.util.spec_from_file_location("make_mme_cases", os.path.join(ROOT, "tests", "golden", "make_mme_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cell(p, edge):
    return np.floor(np.asarray(p, dtype=np.float32).astype(np.float64) / edge).astype(np.int64)


def test_table_holds_what_the_issue_lists(golden):
    assert mc.SIZES == [0, 1, 3, 4, 5, 63, 64, 65, 257]
    for n in mc.SIZES:
        c, g = mc.CASES[f"s{n}"], golden[f"s{n}"]
        assert len(c["cloud"]) == n and c["min_pts"] == 5 and c["radius"] == 0.25 and g["status"] == 0
    assert golden["s4"]["n_dense"] == 0 and np.isnan(golden["s4"]["mme"]) and golden["s257"]["n_scored"] > 200 and golden["s0"]["n_pairs"] == 0
    d = golden["density_edge"]   # the centre with min_pts - 1 neighbours' worth (n = 4) is sparse, the one with n = 5 dense
    assert d["n"].tolist() == [4, 2, 2, 2, 5, 2, 2, 2, 2] and d["cls"].tolist() == [0, 0, 0, 0, mc.SCORED, 0, 0, 0, 0] and d["worst"] == 4
    r = golden["reach_exact"]    # record 1 at d2 == r^2 exactly is a member of record 0's neighbourhood, record 2 one float outward is not
    c = mc.CASES["reach_exact"]["cloud"].astype(np.float64)
    assert (c[1] ** 2).sum() == mc.CASES["reach_exact"]["radius"] ** 2 and (c[2] ** 2).sum() > mc.CASES["reach_exact"]["radius"] ** 2
    assert r["n"][0] == 6 == len(c) - 1 and r["cls"][0] == mc.SCORED   # every record but 2
    assert len(mc.DIRECTIONS) == 26
    for d in mc.DIRECTIONS:      # the query's four-point cluster lies in the neighbour cell the name says; without it the query is sparse
        c, g = mc.CASES[mc.dir_name(d)], golden[mc.dir_name(d)]
        assert c["min_pts"] == 6 and g["n"].tolist() == [6, 1, 1, 5, 5, 5, 5, 2] and g["cls"].tolist() == [mc.SCORED] + [0] * 7
        for k in range(3, 7):
            assert tuple(cell(c["cloud"][k], 0.25) - cell(c["cloud"][0], 0.25)) == d
        assert tuple(cell(c["cloud"][7], 0.25) - cell(c["cloud"][0], 0.25)) == (0, 0, 0)
    assert golden["two_cells_away"]["n"].tolist() == [1, 1, 1, 4, 4, 4, 4] and golden["wrap_trap"]["n"].tolist() == [2, 1, 2]
    hv = mc.CASES["heavy_cell"]["cloud"]
    assert len(hv) == 752 and (cell(hv[2:602], 0.25) == 0).all() and golden["heavy_cell"]["n"][2:602].min() > 300
    z = mc.CASES["around_zero"]["cloud"]
    assert (np.abs(z[:8]) < 1e-6).all() and (z[:8] < 0).any() and (z[:8] > 0).any() and (golden["around_zero"]["n"][:8] >= 16).all()
    dup = golden["duplicates"]
    assert dup["n"][40:44].tolist() == dup["n"][[3, 3, 17, 5]].tolist() and dup["h"][40] == dup["h"][41] == dup["h"][3]
    a = golden["all_duplicates"]
    assert a["n"].tolist() == [8] * 8 and (a["cls"] == mc.FLAT).all() and a["mpv"] == 0.0 and np.isnan(a["mme"]) and a["n_scored"] == 0
    f = mc.CASES["far_clusters"]
    assert f["radius"] == 0.05 and np.linalg.norm(f["cloud"][64:].mean(0) - f["cloud"][:64].mean(0)) > 2900 and golden["far_clusters"]["n_scored"] > 50
    assert mc.CASES["one_cell"]["radius"] > np.ptp(mc.CASES["one_cell"]["cloud"], axis=0).max() and golden["one_cell"]["n_scored"] == 50
    assert golden["plane_noise_1cm"]["n_scored"] >= 140
    t = golden["tilted_plane_1mm"]
    assert t["n_scored"] == 150 and 1e3 < np.median(t["kappa"]) < 1e5                       # det / (tr/3)^3 about 1e-4
    for name in ("plane_exact", "plane_f32_at_50m", "line"):                                # flat: lmin, no h
        g = golden[name]
        assert (g["cls"] == mc.FLAT).all() and g["n_scored"] == 0 and np.isnan(g["mme"]) and g["mpv"] < 1e-12, name
    assert golden["plane_exact"]["mpv"] == 0.0 and (mc.CASES["plane_exact"]["cloud"][:, 2] == 0.25).all()
    assert mc.CASES["plane_f32_at_50m"]["radius"] == 0.3 and mc.CASES["plane_f32_at_50m"]["cloud"].min(0).tolist() >= [50.0, 60.0, 2.0]
    assert mc.CASES["box_far"]["cloud"].min(0).tolist() >= [2999.0, 1999.0, 99.0] and golden["box_far"]["n_scored"] > 100
    for name, st in (("nan_cloud", 1), ("inf_cloud", 1), ("range_at", 2), ("range_below", 0)):
        g = golden[name]
        assert g["status"] == st and (g["n_pairs"] == 0) == bool(st), name
    assert np.abs(mc.CASES["range_at"]["cloud"]).max() / mc.CASES["range_at"]["radius"] == 2.0 ** 30
    assert mc.C_H == 16.0 * max(1.0, mc.NUMPY_RATIO_H) and mc.C_L == 16.0 * max(1.0, mc.NUMPY_RATIO_L) and os.path.getsize(mc.GOLDEN) < 500 << 10


def test_golden_file_regenerates_to_the_bit():
    mod = load_generator()
    again = mod.evaluate(mc.CASES)   # (from the frozen inputs; the generator's assertions run again)
    again.update(mod.inputs(mc.CASES))
    z = np.load(mc.GOLDEN)
    assert sorted(again) == sorted(z.files)
    for k in z.files:
        assert again[k].dtype == z[k].dtype and again[k].shape == z[k].shape and again[k].tobytes() == z[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    fresh = mc.build()
    assert list(fresh) == mc.NAMES
    for name, c in fresh.items():
        f = mc.CASES[name]
        assert c["radius"] == f["radius"] and c["min_pts"] == f["min_pts"], name
        a, b = c["cloud"], f["cloud"]
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), name
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin], b[~fin], equal_nan=True) and np.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-12), name


def test_numpy_statement_is_exact_on_decisions_and_within_c_on_figures(golden):
    mod = load_generator()
    (rh, wh), (rl, wl) = mod.ratios(mc.CASES, golden, cloudmetrics.mme)   # (asserts counts, classes, worst and status exactly)
    print(f"cloudmetrics.mme against the 50-digit figures: h {rh:.3f} at {wh} (NUMPY_RATIO_H {mc.NUMPY_RATIO_H}), lmin {rl:.3f} at {wl} "
          f"(NUMPY_RATIO_L {mc.NUMPY_RATIO_L})")
    assert rh <= mc.C_H and rl <= mc.C_L
    assert rh <= 2.0 * mc.NUMPY_RATIO_H and rl <= 2.0 * mc.NUMPY_RATIO_L


def build_probe(tmp, *flags):
    exe = tmp / ("mme_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *flags, "-o", str(exe), PROBE], check=True, capture_output=True, text=True)
    return exe


def run_probe(exe, tmp, names):
    """The probe over the named cases -> {name: cloudmetrics.mme's dict, with the header fields and seen}."""
    path = tmp / "clouds.bin"
    with open(path, "wb") as f:
        for n in names:
            c = mc.CASES[n]
            f.write(np.float64(c["radius"]).tobytes() + np.array([len(c["cloud"]), c["min_pts"]], dtype=np.uint64).tobytes() + c["cloud"].tobytes())
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), {}, 0
    for n in names:
        h = lines[at].split()
        m = int(h[1])
        assert h[0] == "cloud" and m == len(mc.CASES[n]["cloud"]), lines[at]
        rows = [ln.split() for ln in lines[at + 1:at + 1 + m]]
        rec = lines[at + 1 + m].split()
        assert rec[0] == "record", lines[at + 1 + m]
        out[n] = dict(status=int(h[3]), edge=float.fromhex(h[5]), doublings=int(h[7]), cells=[int(v) for v in h[9:12]],
                      n=np.array([int(r[0]) for r in rows], dtype=np.uint32), cls=np.array([int(r[1]) for r in rows], dtype=np.uint8),
                      h=np.array([float.fromhex(r[2]) if "nan" not in r[2] else np.nan for r in rows], dtype=np.float64),
                      lmin=np.array([float.fromhex(r[3]) if "nan" not in r[3] else np.nan for r in rows], dtype=np.float64),
                      seen=np.array([int(r[4]) for r in rows], dtype=np.int64),
                      mme=float.fromhex(rec[1]) if "nan" not in rec[1] else np.nan, mpv=float.fromhex(rec[2]) if "nan" not in rec[2] else np.nan,
                      h_max=float.fromhex(rec[3]) if "nan" not in rec[3] else np.nan, n_dense=int(rec[4]), n_scored=int(rec[5]), n_pairs=int(rec[6]),
                      worst=int(rec[7]))
        at += 2 + m
    return out


def seen_by_floor(cloud, edge):
    """Records in the 27 cells around each record's own, cells by floor: what a walk has to look at and no more."""
    k = cell(cloud, edge)
    near = (np.abs(k[:, None, :] - k[None, :, :]) <= 1).all(axis=2)
    return near.sum(axis=1)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mme_probe")
    return tmp, build_probe(tmp)


def test_device_route_on_the_host_under_sanitizers(golden, brute, probe):
    """The CPU twin on every case: clean under the sanitizers, counts and classes those of the numpy statement and of the table exactly, figures
    within tolerance; the edge doubled exactly as often as it had to."""
    tmp, exe = probe
    got = run_probe(exe, tmp, mc.NAMES)
    mod = load_generator()
    twin = lambda cloud, radius, min_pts: got[next(n for n, c in mc.CASES.items() if c["cloud"] is cloud)]   # noqa: E731
    for name in mc.NAMES:
        g, b = got[name], brute[name]
        assert g["status"] == golden[name]["status"] == b["status"], name
        assert np.array_equal(g["n"], b["n"]) and np.array_equal(g["cls"], b["cls"]), name
        assert (g["n_dense"], g["n_scored"], g["n_pairs"], g["worst"]) == (b["n_dense"], b["n_scored"], b["n_pairs"], b["worst"]), name
    (rh, wh), (rl, wl) = mod.ratios(mc.CASES, golden, twin)
    print(f"the host twin against the 50-digit figures: h {rh:.3f} at {wh}, lmin {rl:.3f} at {wl} (C_H {mc.C_H}, C_L {mc.C_L})")
    assert rh <= mc.C_H and rl <= mc.C_L
    for name, c in mc.CASES.items():
        if not golden[name]["status"] and got[name]["doublings"] == 0:
            assert np.array_equal(got[name]["seen"], seen_by_floor(c["cloud"], c["radius"])), name
    far, one = got["far_clusters"], got["one_cell"]
    assert far["doublings"] >= 1 and far["edge"] == 0.05 * 2.0 ** far["doublings"] and np.prod(np.array(far["cells"], dtype=np.float64)) < 2.0 ** 31
    p64 = mc.CASES["far_clusters"]["cloud"].astype(np.float64)
    cells = lambda edge: np.floor(p64.max(0) / edge) - np.floor(p64.min(0) / edge) + 1   # noqa: E731
    assert cells(far["edge"]).tolist() == far["cells"] and np.prod(cells(far["edge"] / 2)) >= 2.0 ** 31   # ... and not once more than it had to
    assert np.array_equal(far["seen"], seen_by_floor(mc.CASES["far_clusters"]["cloud"], far["edge"]))
    assert one["cells"] == [1, 1, 1] and one["doublings"] == 0 and (one["seen"] == 50).all()
    assert got["range_below"]["doublings"] == 0 and got["range_below"]["cells"][0] > 2 ** 29 and got["range_at"]["n"].tolist() == [0, 0, 0]
    assert got["wrap_trap"]["cells"] == [6, 2, 1] and got["wrap_trap"]["seen"].tolist() == [2, 1, 2]   # A does not look at B, first cell of the next row
    assert got["around_zero"]["cells"] == [4, 4, 4]
    bad = subprocess.run([str(exe), str(tmp / "missing.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "cannot open" in bad.stderr
    (tmp / "short.bin").write_bytes(np.float64(0.25).tobytes() + np.array([3, 5], dtype=np.uint64).tobytes() + b"\0" * 8)
    bad = subprocess.run([str(exe), str(tmp / "short.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "truncated" in bad.stderr


def test_truncation_in_the_place_of_floor_fails_around_zero(probe):
    """-DMME_HOST_TRUNC: -1e-7 then lies in cell 0 with +1e-7, the cell at 0 is two edges wide and the grid a cell short per axis.  Every neighbour is
    still found - a wider cell only costs work - so what fails is the grid's shape and the records looked at."""
    tmp, _ = probe
    got = run_probe(build_probe(tmp, "-DMME_HOST_TRUNC"), tmp, ["around_zero"])["around_zero"]
    c = mc.CASES["around_zero"]
    assert got["cells"] == [3, 3, 3] and got["cells"] != [4, 4, 4]
    want = seen_by_floor(c["cloud"], c["radius"])
    assert (got["seen"] >= want).all() and (got["seen"][:8] > want[:8]).all()


def variant(cloud, radius, min_pts, about_origin=False, biased=False, no_self=False, strict=False, no_floor=False):
    """cloudmetrics.mme with one thing wrong."""
    p = np.asarray(cloud, dtype=np.float32).astype(np.float64)
    m = len(p)
    out = dict(n=np.zeros(m, dtype=np.uint32), cls=np.zeros(m, dtype=np.uint8), h=np.full(m, np.nan))
    for i in range(m):
        d = p[i] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = d2 < radius * radius if strict else d2 <= radius * radius
        if no_self:
            inside[i] = False
        u = p[inside] if about_origin else -d[inside]
        n = len(u)
        out["n"][i] = n
        if n < min_pts:
            continue
        s, mm = u.sum(0), u.T @ u
        c = (mm - np.outer(s, s) / n) / (n if biased else n - 1)
        det = c[0, 0] * (c[1, 1] * c[2, 2] - c[1, 2] * c[1, 2]) - c[0, 1] * (c[0, 1] * c[2, 2] - c[1, 2] * c[0, 2]) + c[0, 2] * (c[0, 1] * c[1, 2] - c[1, 1] * c[0, 2])
        flat = det <= (0.0 if no_floor else mc.FLOOR * (np.trace(c) / 3.0) ** 3)
        out["cls"][i] = mc.FLAT if flat else mc.SCORED
        if not flat:
            out["h"][i] = 0.5 * (cloudmetrics.LN_2PIE_3 + np.log(det))
    return out


def h_within(name, golden, got):
    g = golden[name]
    sc = g["cls"] == mc.SCORED
    return np.array_equal(got["cls"], g["cls"]) and bool((np.abs(got["h"][sc] - g["h"][sc]) <= mc.tol_h(g)[sc]).all())


@pytest.mark.parametrize("name,wrong", [("box_far", "about_origin"), ("s257", "biased"), ("density_edge", "no_self"), ("reach_exact", "strict"),
                                        ("plane_f32_at_50m", "no_floor")])
def test_wrong_variants_of_the_restatement_fail_on_a_named_case(golden, name, wrong):
    c = mc.CASES[name]
    right = variant(c["cloud"], c["radius"], c["min_pts"])
    assert np.array_equal(right["n"], golden[name]["n"]) and h_within(name, golden, right), "the variant without a fault agrees"
    got = variant(c["cloud"], c["radius"], c["min_pts"], **{wrong: True})
    if wrong in ("no_self", "strict"):
        assert not np.array_equal(got["n"], golden[name]["n"])
    elif wrong == "no_floor":
        assert np.array_equal(got["n"], golden[name]["n"]) and (got["cls"] == mc.SCORED).any() and (golden[name]["cls"] == mc.FLAT).all()
    else:
        assert np.array_equal(got["n"], golden[name]["n"]) and not h_within(name, golden, got)


def test_kd_tree_counts_the_same_neighbours(golden):
    spatial = pytest.importorskip("scipy.spatial")
    n = 0
    for name, c in mc.CASES.items():
        g = golden[name]
        if g["status"] or not len(c["cloud"]) or name == "reach_exact":   # (the tree compares distances, not d2: no promise on an exact tie)
            continue
        p64 = c["cloud"].astype(np.float64)
        cnt = spatial.cKDTree(p64).query_ball_point(p64, c["radius"], return_length=True)
        assert np.array_equal(cnt, g["n"]), name
        n += len(p64)
    assert n > 2000


def test_mme_record_is_64_bytes():
    assert C.sizeof(abi.lk_mme) == 64 and abi.mme_dtype().itemsize == 64
    assert [f for f, _ in abi.lk_mme._fields_] == FIELDS == list(abi.mme_dtype().names)
    assert (abi.LK_MME_NONFINITE, abi.LK_MME_RANGE) == (cloudmetrics.LK_MME_NONFINITE, cloudmetrics.LK_MME_RANGE)
    assert (cloudmetrics.MME_SPARSE, cloudmetrics.MME_FLAT, cloudmetrics.MME_SCORED) == (mc.SPARSE, mc.FLAT, mc.SCORED) and cloudmetrics.MME_FLOOR == mc.FLOOR


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + " %u %u\\n\", sizeof(lk_mme), "
                   + ", ".join(f"offsetof(lk_mme, {f})" for f in FIELDS) + ", LK_MME_NONFINITE, LK_MME_RANGE); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 64
    assert got[1:10] == [getattr(abi.lk_mme, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert got[1:10] == [abi.mme_dtype().fields[f][1] for f in FIELDS]
    assert got[10:12] == [abi.LK_MME_NONFINITE, abi.LK_MME_RANGE] == [1, 2]


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS and s in sigs and len(sigs[s][1]) == 10
        assert sigs[s][1][2:6] == [C.c_size_t, C.c_void_p, C.c_double, C.c_uint32]
    assert callable(binding.LegKiloHip.clouds_mme_dev) and callable(binding.LegKiloHip.clouds_mme)
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for phrase in ("d2(i, j) <= r * r", "ABOUT THE QUERY POINT", "C = (M - s s^T / n_i) / (n_i - 1)", "det <= 2^-30 * (tr / 3)^3", "h_i = 0.5 * (3 * ln(2 pi e) + ln det)",
                   "LK_MME_RANGE"):
        assert phrase in hdr, phrase   # the definition the tests implement stands in the header


def test_host_header_compiles_with_the_new_wrapper(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::cloudsMmeDev;\nint main() { return a ? 0 : 1; }\n')
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
