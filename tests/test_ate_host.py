"""CPU checks of the trajectory-error entries (lk_traj_ate_dev / lk_runs_ate_dev): the case table of tests/atecases.py against its 50-digit values,
the association rule against tum.associate, leg-kilo_amd/csrc/lk_horn.h compiled for the host (tools/probes/horn_host.cc) on every case's
cross-covariance, deliberately wrong restatements that must each fail on a named case, the same probe as a stand-alone program under the address and
undefined-behaviour sanitizers, and the C-ABI: lk_ate's size and field offsets from a C program compiled against the header, the exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import ate_ref
import atecases as ac
from legkilo_amd import abi, binding, tum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ate_cases.npz")
PROBE = os.path.join(ROOT, "tools", "probes", "horn_host.cc")
NEW_SYMBOLS = ["lk_traj_ate_dev", "lk_runs_ate_dev"]
FIELDS = ["rmse", "mean", "max", "rot", "trans", "n_pairs", "worst", "status"]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def expected(golden, name, flag):
    k = f"{name}/a{flag}/"
    fig, cnt = golden[k + "figures"], golden[k + "counts"]
    return dict(rmse=fig[0], mean=fig[1], max=fig[2], n_pairs=int(cnt[0]), status=int(cnt[1]), worst=int(cnt[2]), worst_margin=float(golden[k + "worst_margin"][0]),
                pairs=golden[k + "pairs"])


def figures_ratio(got, want, c):
    """Largest |x - x_50| / (2^-53 S) over rmse, mean, max; NaN must meet NaN."""
    worst = 0.0
    for f in ("rmse", "mean", "max"):
        if np.isnan(want[f]):
            assert np.isnan(got[f]), f
        else:
            assert np.isfinite(got[f]), f
            worst = max(worst, abs(float(got[f]) - float(want[f])) / (ac.ULP * ac.scale(c)))
    return worst


def test_table_holds_what_the_issue_lists():
    assert [f"n{n}" for n in ac.SIZES] == ac.NAMES[:len(ac.SIZES)]
    for name in ("empty_est", "empty_gt", "single_gt", "midway", "dt_exact", "outside", "dup_gt", "rate_500_100", "arc_origin", "arc_3p6km", "arc_600km", "planar",
                 "mirrored", "collinear", "coincident2", "identical", "nan_paired", "nan_unpaired"):
        assert name in ac.CASES
    assert len(ac.CASES["empty_est"]["est_t"]) == 0 and len(ac.CASES["empty_gt"]["gt_t"]) == 0 and len(ac.CASES["single_gt"]["gt_t"]) == 1
    assert 3e3 < ac.scale(ac.CASES["arc_3p6km"]) < 4e3 and 5e5 < ac.scale(ac.CASES["arc_600km"]) < 7e5
    assert ac.C == 16.0 * max(1.0, ac.NUMPY_RATIO)


def test_golden_file_regenerates_to_the_bit(golden):
    spec = importlib.util.spec_from_file_location("make_ate_cases", os.path.join(ROOT, "tests", "golden", "make_ate_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    again = mod.evaluate(ac.CASES)   # (from the frozen inputs)
    assert sorted(again) == sorted(k for k in golden if "/a0/" in k or "/a1/" in k)
    for k, v in again.items():
        assert v.dtype == golden[k].dtype and v.shape == golden[k].shape and v.tobytes() == golden[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    """build() gives the table the file froze: names, order, shapes, NaNs, and the values to a few ulp (cos, sin and the normal variates are the
    platform's)."""
    fresh = ac.build()
    assert list(fresh) == ac.NAMES
    for name, c in fresh.items():
        assert c["max_dt"] == ac.CASES[name]["max_dt"], name
        for k in ac.KEYS:
            a, b = c[k], ac.CASES[name][k]
            assert a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(np.isnan(a), np.isnan(b)), (name, k)
            assert np.allclose(a, b, rtol=1e-14, atol=1e-14, equal_nan=True), (name, k)


def test_paired_sizes_and_special_pairs(golden):
    for n in ac.SIZES:
        assert expected(golden, f"n{n}", 1)["n_pairs"] == n
    pairs = lambda name: [tuple(p) for p in expected(golden, name, 0)["pairs"]]   # noqa: E731
    assert pairs("midway") == [(i, i) for i in range(5)]                            # midway between j and j + 1: the earlier
    assert pairs("dt_exact") == [(0, 1), (2, 3), (4, 5)]                            # |dt| == max_dt counts, one ulp above does not
    assert pairs("dup_gt") == [(0, 0), (1, 1), (2, 2), (3, 4), (4, 4), (5, 4), (6, 7), (7, 7)]
    assert pairs("outside") == [(1, 0)] + [(i + 1, i) for i in range(1, 8)] + [(9, 8)]
    assert pairs("single_gt") == [(i, 0) for i in range(5)]
    assert expected(golden, "rate_500_100", 0)["n_pairs"] == 26 and expected(golden, "rate_500_100_wide", 0)["n_pairs"] == 126
    assert expected(golden, "nan_paired", 1)["status"] == 1 and expected(golden, "nan_unpaired", 1)["status"] == 0
    assert expected(golden, "nan_unpaired", 1)["n_pairs"] == 19
    z = expected(golden, "identical", 0)
    assert (z["rmse"], z["mean"], z["max"]) == (0.0, 0.0, 0.0)


def test_numpy_restatement_against_50_digits(golden):
    """Every case, both flags: pairs, n_pairs, status exact; figures within C; the measured ratio is the one C was derived from."""
    worst, where = 0.0, None
    for name in ac.NAMES:
        c = ac.CASES[name]
        for flag in ac.FLAGS:
            want, got = expected(golden, name, flag), ate_ref.ate(c, flag)
            assert np.array_equal(got["pairs"], want["pairs"]), (name, flag)
            assert (got["n_pairs"], got["status"]) == (want["n_pairs"], want["status"]), (name, flag)
            r = figures_ratio(got, want, c)
            assert r <= ac.C, (name, flag, r)
            if want["n_pairs"] and not want["status"] and want["worst_margin"] > 2 * ac.tol(c):
                assert got["worst"] == want["worst"], (name, flag)
            if flag and want["n_pairs"] and not want["status"]:   # the restatement's rmse IS tum.ate's
                g, p = c["gt_pos"][got["pairs"][:, 1]], c["est_pos"][got["pairs"][:, 0]]
                assert got["rmse"] == tum.ate(g, p, align=True)
                assert abs(float(np.sqrt((got["e"] ** 2).mean())) - got["rmse"]) <= 4 * ac.ULP * ac.scale(c)
            if r > worst:
                worst, where = r, (name, flag)
    print(f"numpy restatement: worst ratio {worst:.3f} at {where}; NUMPY_RATIO {ac.NUMPY_RATIO}, C {ac.C}")
    assert worst <= 2 * ac.NUMPY_RATIO, f"measured {worst} at {where}: tests/atecases.py's NUMPY_RATIO (and with it C) is stale"
    assert ac.CASES["identical"] and ate_ref.ate(ac.CASES["identical"], 0)["rmse"] == 0.0


def spaced(c):
    """Consecutive stamps of BOTH trajectories more than 2 max_dt apart: the header's condition for tum.associate's pairs."""
    return all(len(t) < 2 or np.diff(t).min() > 2 * c["max_dt"] for t in (c["est_t"], c["gt_t"]))


def test_pairs_are_tum_associates_where_the_stamps_are_spaced(golden):
    same = []
    for name in ac.NAMES:
        c = ac.CASES[name]
        if spaced(c):
            want = tum.associate(c["est_t"], c["gt_t"], c["max_dt"])
            assert np.array_equal(ate_ref.associate(c["est_t"], c["gt_t"], c["max_dt"]), want), name
            same.append(name)
    for name in ["n0", "n65", "n257", "arc_600km", "outside", "nan_unpaired", "dt_exact"]:
        assert name in same, name
    assert len(same) >= 20
    c = ac.CASES["rate_500_100_wide"]   # 2 ms between estimate stamps, max_dt 5 ms: a ground-truth sample serves five, tum.associate uses each once
    assert not spaced(c)
    ours, theirs = ate_ref.associate(c["est_t"], c["gt_t"], c["max_dt"]), tum.associate(c["est_t"], c["gt_t"], c["max_dt"])
    assert len(ours) == 126 and len(theirs) < len(ours) and len(np.unique(theirs[:, 1])) == len(theirs) and len(np.unique(ours[:, 1])) < len(ours)


@pytest.fixture(scope="module")
def horn(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("horn") / "horn_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-o", so, PROBE])
    L = C.CDLL(so)

    def run(S):
        S = np.ascontiguousarray(S, dtype=np.float64).reshape(-1, 9)
        R = np.zeros_like(S)
        L.lk_horn_rotation_host_n(S.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int(len(S)))
        return R.reshape(-1, 3, 3)

    return run


def test_horn_solver_on_every_cross_covariance(golden, horn):
    """lk_horn.h on the centred cross-covariance of every case's pairs: a proper rotation, orthonormal to 1e-14, whose rmse is the 50-digit one within C."""
    worst, where, n = 0.0, None, 0
    for name in ac.NAMES:
        c, want = ac.CASES[name], expected(golden, name, 1)
        if not want["n_pairs"] or want["status"]:
            continue
        g, p = c["gt_pos"][want["pairs"][:, 1]], c["est_pos"][want["pairs"][:, 0]]
        cg, cp = g.mean(0), p.mean(0)
        R = horn((p - cp).T @ (g - cg))[0]
        assert abs(np.linalg.det(R) - 1.0) <= 1e-14, name
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14, name
        d = (g - cg) - (p - cp) @ R.T
        r = abs(float(np.sqrt((d * d).sum(1).mean())) - want["rmse"]) / (ac.ULP * ac.scale(c))
        assert r <= ac.C, (name, r)
        n += 1
        if r > worst:
            worst, where = r, name
    print(f"lk_horn.h over {n} cases: worst rmse ratio {worst:.3f} at {where} (C {ac.C})")
    assert n >= 20
    assert np.array_equal(horn(np.zeros(9))[0], np.eye(3)) and np.array_equal(horn(np.full(9, np.nan))[0], np.eye(3))


def test_wrong_variants_each_fail_on_a_named_case(golden):
    """The table tells a wrong implementation from a right one: each variant misses on the case made for it - and the right one does not."""
    def misses(name, flag, variant):
        c, want = ac.CASES[name], expected(golden, name, flag)
        got = ate_ref.ate(c, flag, variant)
        if not np.array_equal(got["pairs"], want["pairs"]):
            return "pairs"
        return "figures" if figures_ratio(got, want, c) > ac.C else None

    assert misses("mirrored", 1, "no_det") == "figures"          # the reflection fits a mirrored trajectory to the noise: orders of magnitude off
    assert ate_ref.ate(ac.CASES["mirrored"], 1, "no_det")["rmse"] < 1e-6 < 0.1 < expected(golden, "mirrored", 1)["rmse"]
    assert misses("arc_600km", 1, "one_pass") == "figures"       # sum x y - n mean mean at 600 km
    assert misses("arc_3p6km", 1, "one_pass") == "figures"
    assert misses("dt_exact", 0, "strict") == "pairs"            # < instead of <=
    assert misses("midway", 0, "later") == "pairs"               # ties to the later sample
    assert misses("dup_gt", 0, "later") == "pairs"
    for name, flag in (("mirrored", 1), ("arc_600km", 1), ("arc_3p6km", 1), ("dt_exact", 0), ("midway", 0), ("dup_gt", 0)):
        assert misses(name, flag, None) is None, name


def test_horn_probe_under_the_host_sanitizers(tmp_path):
    """tools/probes/horn_host.cc with its own main: -fsanitize=address,undefined, the runtimes linked statically (nothing is loaded into this process)."""
    exe = tmp_path / "horn_host"
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-DLK_HORN_MAIN", PROBE, "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "horn ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_ate_record_is_136_bytes():
    assert C.sizeof(abi.lk_ate) == 136 and abi.ate_dtype().itemsize == 136
    assert [f for f, _ in abi.lk_ate._fields_] == FIELDS == list(abi.ate_dtype().names)


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + " %u %u\\n\", sizeof(lk_ate), "
                   + ", ".join(f"offsetof(lk_ate, {f})" for f in FIELDS) + ", LK_ATE_ALIGN, LK_ATE_NONFINITE); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 136
    assert got[1:9] == [getattr(abi.lk_ate, f).offset for f in FIELDS] == [0, 8, 16, 24, 96, 120, 128, 132]
    assert got[1:9] == [abi.ate_dtype().fields[f][1] for f in FIELDS]
    assert got[9:] == [abi.LK_ATE_ALIGN, abi.LK_ATE_NONFINITE] == [1, 1]


def test_symbols_are_exported_and_the_abi_version_stays():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
