"""CPU checks of the relative-pose-error entries (lk_traj_rpe_dev / lk_runs_rpe_dev): the case table of tests/rpecases.py against its 50-digit values
through the numpy restatement legkilo_amd.tum.rpe, deliberately wrong restatements that must each fail on a named case, leg-kilo_amd/csrc/lk_relpose.h
compiled for the host as a stand-alone program (tools/probes/relpose_host.cc) under the address and undefined-behaviour sanitizers on every term of
the table, tum.quat_to_rot, the C++ wrappers, and the C-ABI: lk_rpe's size and field offsets from a C program compiled against the header, the
exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import rpe_ref
import rpecases as rc
from legkilo_amd import abi, binding, tum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "relpose_host.cc")
NEW_SYMBOLS = ["lk_traj_rpe_dev", "lk_runs_rpe_dev"]
FIELDS = ["trans_rmse", "trans_mean", "trans_max", "rot_rmse", "rot_mean", "rot_max", "n_terms", "n_pairs", "worst_trans", "worst_rot", "status", "reserved"]


@pytest.fixture(scope="module")
def golden():
    return rc.golden()


def all_modes():
    return [(name, q, delta, flags) for name in rc.NAMES for q, delta, flags in rc.modes(rc.CASES[name])]


def test_table_holds_what_the_issue_lists(golden):
    assert [f"n{n}" for n in rc.SIZES] == rc.NAMES[:len(rc.SIZES)] and rc.SIZES == [0, 1, 2, 63, 64, 65, 129, 257]
    for n in rc.SIZES:
        assert len(rc.CASES[f"n{n}"]["est_t"]) == n
    for name in ("empty_gt", "step_edges", "step_past_end", "step_small", "dup_swallow", "unpaired_ends", "gt_fifth", "dt_edges", "dt_edges_before", "midway",
                 "identical", "rigid_yaw2_km", "rigid_tilt", "noisy_origin", "noisy_3p6km", "noisy_600km", "noisy_rigid", "rot_angles", "rot_180_exact",
                 "rot_1e-9", "gt_scaled", "pure_rotation", "pure_translation", "const_step", "nan_pos_term", "nan_rot_term", "nan_unpaired", "nan_no_term"):
        assert name in rc.CASES, name
    assert len(rc.CASES["empty_gt"]["gt_t"]) == 0 and len(rc.CASES["n0"]["est_t"]) == 0 and len(rc.CASES["n0"]["gt_t"]) > 0
    assert sorted(int(d) for d, f in rc.CASES["n129"]["modes"] if f) == [1, 63, 64, 65, 129, 500]
    E = lambda name, q: rc.expected(golden, name, q)   # noqa: E731
    assert 3e3 < E("noisy_3p6km", 0)["S"] < 4e3 and 5e5 < E("noisy_600km", 0)["S"] < 7e5 and 3e3 < E("rigid_yaw2_km", 0)["S"] < 4e3
    assert E("noisy_origin", 0)["S"] < 10 and E("gt_scaled", 0)["M"] == pytest.approx(1.0 + 1e-6, abs=1e-9)
    assert rc.C_T == 16.0 * rc.NUMPY_RATIO_T and rc.C_R == 16.0 * rc.NUMPY_RATIO_R
    assert os.path.getsize(rc.GOLDEN) < 200 << 10


def test_step_and_pairing_cases_give_the_terms_they_were_built_for(golden):
    T = lambda name, q: [tuple(int(x) for x in t) for t in rc.expected(golden, name, q)["terms"]]   # noqa: E731
    E = lambda name, q: rc.expected(golden, name, q)                                                # noqa: E731
    # t_i + delta == t_k exactly: k = i + 2; from i = 2 the target lies one ulp above t[4]: k = 5
    assert [(i, k) for i, k, _, _ in T("step_edges", 0)] == [(0, 2), (1, 3), (2, 5), (3, 5), (4, 6), (5, 7), (6, 8), (7, 9), (8, 10), (9, 11)]
    for q in (0, 1):
        assert (E("step_past_end", q)["n_terms"], E("step_past_end", q)["n_pairs"]) == (0, 12)
        assert np.isnan(E("step_past_end", q)["trans_rmse"]) and E("step_past_end", q)["status"] == 0
    assert T("step_small", 0) == T("step_small", 1) == [(i, i + 1, i, i + 1) for i in range(11)]
    # duplicate stamps and a delta the addition swallows: still the next sample; equal stamps share the earliest partner, so a == b occurs
    assert T("dup_swallow", 0) == [(0, 1, 0, 0), (1, 2, 0, 0), (2, 3, 0, 1), (3, 4, 1, 1), (4, 5, 1, 2), (5, 6, 2, 3), (6, 7, 3, 3), (7, 8, 3, 3), (8, 9, 3, 4)]
    # samples 5, 9, 10 unpaired: no term starts or ends there
    assert [(i, k) for i, k, _, _ in T("unpaired_ends", 1)] == [(0, 1), (1, 2), (2, 3), (3, 4), (6, 7), (7, 8), (11, 12), (12, 13)]
    assert E("unpaired_ends", 1)["n_pairs"] == 11
    assert any(a == b for _, _, a, b in T("gt_fifth", 0)) and any(a != b for _, _, a, b in T("gt_fifth", 0)) and E("gt_fifth", 0)["n_pairs"] == 31
    # |dt| == max_dt pairs, one ulp above does not (samples 2, 5 / 3, 6)
    assert [(i, k) for i, k, _, _ in T("dt_edges", 1)] == [(0, 1), (3, 4), (6, 7)] and E("dt_edges", 1)["n_pairs"] == 6
    assert [(i, k) for i, k, _, _ in T("dt_edges_before", 1)] == [(0, 1), (1, 2), (4, 5)] and E("dt_edges_before", 1)["n_pairs"] == 6
    assert T("midway", 1) == [(i, i + 1, i, i + 1) for i in range(6)]
    # index steps: 65 samples under a step of 64 have one term, 129 under 129 or 500 none
    assert T("n65", 2) == [(0, 64, 0, 64)]
    by_step = {int(d): q for q, d, f in rc.modes(rc.CASES["n129"]) if f}
    assert [E("n129", by_step[s])["n_terms"] for s in (1, 63, 64, 65, 129, 500)] == [128, 66, 65, 64, 0, 0]
    assert [E(f"n{n}", 1)["n_terms"] for n in (0, 1, 2, 63, 64, 65)] == [0, 0, 1, 62, 63, 64] and E("n1", 1)["n_pairs"] == 1
    assert (E("empty_gt", 0)["n_terms"], E("empty_gt", 0)["n_pairs"]) == (0, 0)
    # non-finite values: inside a term they set the status, outside they are invisible
    for name, status in (("nan_pos_term", 1), ("nan_rot_term", 1), ("nan_unpaired", 0), ("nan_no_term", 0)):
        for q in (0, 1):
            e = E(name, q)
            assert e["status"] == status and e["n_terms"] > 0 and np.isnan(e["trans_rmse"]) == bool(status), (name, q)
    assert T("nan_no_term", 1) == [(i, i + 15, i, i + 15) for i in range(5)]
    # geometry
    for q, _, _ in rc.modes(rc.CASES["identical"]):
        assert [E("identical", q)[f] for f in rc.FIGURES] == [0.0] * 6 and E("identical", q)["n_terms"] > 0
    ang = E("rot_angles", 1)["e_r"]
    assert np.allclose(ang[:4], [1e-9, np.pi / 2, np.deg2rad(179.9), np.pi], rtol=1e-7, atol=0) and E("rot_180_exact", 0)["rot_max"] == np.pi
    assert len(set(E("const_step", 0)["e_t"])) == 1 and E("const_step", 0)["e_t"][0] == 2.0 ** -7 and not E("const_step", 0)["e_r"].any()
    for q in (0, 1):   # the frame does not matter: the rigidly moved noisy estimate scores what the unmoved one does
        a, b = E("noisy_origin", q), E("noisy_rigid", q)
        for f in rc.FIGURES:
            assert abs(a[f] - b[f]) <= 64 * rc.ULP * b["S"], (q, f)   # (b's inputs were rounded at 3.6 km)
        assert (a["worst_trans"], a["worst_rot"]) == (b["worst_trans"], b["worst_rot"])


def test_golden_file_regenerates_to_the_bit(golden):
    spec = importlib.util.spec_from_file_location("make_rpe_cases", os.path.join(ROOT, "tests", "golden", "make_rpe_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    again = mod.evaluate(rc.CASES)   # (from the frozen inputs)
    assert sorted(again) == sorted(k for k in golden if "/in/" not in k)
    for k, v in again.items():
        assert v.dtype == golden[k].dtype and v.shape == golden[k].shape and v.tobytes() == golden[k].tobytes(), k
    mod.check_worst(rc.CASES, golden)
    packed = rc.pack(golden)
    z = np.load(rc.GOLDEN)
    assert sorted(packed) == sorted(z.files)
    for k in packed:
        assert packed[k].dtype == z[k].dtype and packed[k].tobytes() == z[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    """build() gives the table the file froze: names, order, shapes, NaNs, and the values to a few ulp (cos, sin and the normal variates are the
    platform's)."""
    fresh = rc.build()
    assert list(fresh) == rc.NAMES
    for name, c in fresh.items():
        assert c["max_dt"] == rc.CASES[name]["max_dt"] and np.array_equal(c["modes"], rc.CASES[name]["modes"]), name
        for k in rc.KEYS:
            a, b = c[k], rc.CASES[name][k]
            assert a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(np.isfinite(a), np.isfinite(b)), (name, k)
            assert np.allclose(a, b, rtol=1e-14, atol=1e-14, equal_nan=True), (name, k)


def test_numpy_restatement_against_50_digits(golden):
    """Every case, every mode: term list, counts, status exact; figures and term values within C; worst_* by the table's rule; the measured ratios
    are the ones C_T and C_R were derived from."""
    worst, where = [0.0, 0.0], [None, None]
    for name, q, delta, flags in all_modes():
        c, want = rc.CASES[name], rc.expected(golden, name, q)
        got = rpe_ref.rpe(c, delta, flags)
        assert np.array_equal(got["terms"], want["terms"]), (name, q)
        ratios = rc.check(name, got, want)
        if want["n_terms"] and not want["status"]:
            ratios[0] = max(ratios[0], float(np.abs(got["e_t"] - want["e_t"]).max()) / (rc.ULP * want["S"]))
            ratios[1] = max(ratios[1], float(np.abs(got["e_r"] - want["e_r"]).max()) / (rc.ULP * want["M"] ** 2))
        for h in (0, 1):
            if ratios[h] > worst[h]:
                worst[h], where[h] = ratios[h], (name, q)
    print(f"numpy restatement: worst ratios {worst[0]:.3f} at {where[0]} (NUMPY_RATIO_T {rc.NUMPY_RATIO_T}), {worst[1]:.3f} at {where[1]} (NUMPY_RATIO_R {rc.NUMPY_RATIO_R})")
    assert worst[0] <= 2 * rc.NUMPY_RATIO_T and worst[1] <= 2 * rc.NUMPY_RATIO_R, f"measured {worst} at {where}: tests/rpecases.py's NUMPY_RATIO_* (and with them C_*) are stale"
    z = rpe_ref.rpe(rc.CASES["identical"], 1.0, 1)
    assert [z[f] for f in rc.FIGURES] == [0.0] * 6


def test_wrong_variants_each_fail_on_a_named_case(golden):
    """The table tells a wrong implementation from a right one: each variant misses on the case made for it - and the right one does not."""
    def misses(name, q, variant):
        c, want = rc.CASES[name], rc.expected(golden, name, q)
        _, delta, flags = rc.modes(c)[q]
        got = rpe_ref.rpe(c, delta, flags, variant)
        if not np.array_equal(got["terms"], want["terms"]):
            return "terms"
        try:
            rc.check(name, got, want)
        except AssertionError:
            return "figures"
        return None

    made_for = [("dup_swallow", 0, "from0", "terms"),        # target == t_i: the search from 0 ends at i or at an earlier equal stamp
                ("step_edges", 0, "strict", "terms"),        # t_i + delta == t_k exactly
                ("midway", 1, "later", "terms"),             # a tie between two ground-truth samples
                ("rigid_yaw2_km", 0, "world", "figures"),    # a yaw of 2 rad turns every world-frame displacement
                ("noisy_rigid", 1, "world", "figures"),
                ("rot_1e-9", 1, "acos", "figures"),          # acos resolves 1.5e-8 rad near c = 1
                ("gt_scaled", 0, "reortho", "figures")]      # the formula on the bits as given, not the "true angle"
    for name, q, variant, how in made_for:
        assert misses(name, q, variant) == how, (name, q, variant)
        assert misses(name, q, None) is None, (name, q)
    assert sorted({v for _, _, v, _ in made_for}) == sorted(rpe_ref.VARIANTS)


@pytest.fixture(scope="module")
def relpose(tmp_path_factory):
    """tools/probes/relpose_host.cc as a program of its own: -fsanitize=address,undefined, the runtimes linked statically (nothing is loaded into this
    process).  run(cases [n, 48]) -> [n, 4]: e_t, s, c, e_r."""
    d = tmp_path_factory.mktemp("relpose")
    exe = d / "relpose_host"
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", PROBE, "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)

    def run(cases, through_stdin=False):
        text = "".join(" ".join(float(v).hex() for v in row) + "\n" for row in np.asarray(cases, dtype=np.float64).reshape(-1, 48))
        if through_stdin:
            r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        else:
            (d / "cases.txt").write_text(text)
            r = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        return np.array([[float.fromhex(v) for v in line.split()] for line in r.stdout.splitlines()]).reshape(-1, 4)

    run.exe = exe
    return run


def term_rows(c, terms):
    pose = lambda side, j: np.r_[c[side + "_rot"][j].ravel(), c[side + "_pos"][j]]   # noqa: E731
    return np.array([np.r_[pose("est", i), pose("est", k), pose("gt", a), pose("gt", b)] for i, k, a, b in terms]).reshape(-1, 48)


def test_relpose_header_on_the_host_under_sanitizers(golden, relpose):
    """lk_relpose.h on every finite term of the table: clean under the sanitizers, within C of the 50-digit term values and of tum.rpe's, exactly 0
    for equal poses."""
    worst, n = [0.0, 0.0], 0
    for name, q, delta, flags in all_modes():
        c, want = rc.CASES[name], rc.expected(golden, name, q)
        if not want["n_terms"] or want["status"]:
            continue
        out = relpose(term_rows(c, want["terms"]))
        ref = rpe_ref.rpe(c, delta, flags)
        assert len(out) == want["n_terms"]
        for h, (col, e, unit, cc) in enumerate(((0, "e_t", rc.ULP * want["S"], rc.C_T), (3, "e_r", rc.ULP * want["M"] ** 2, rc.C_R))):
            r = float(np.abs(out[:, col] - want[e]).max()) / unit
            assert r <= cc, (name, q, e, r)
            assert float(np.abs(out[:, col] - ref[e]).max()) / unit <= cc, (name, q, e)
            worst[h] = max(worst[h], r)
        if name == "identical":
            assert not out[:, [0, 1, 3]].any(), (name, q)   # e_t, s and e_r exactly 0.0
        n += len(out)
    print(f"lk_relpose.h over {n} terms: worst ratios {worst[0]:.3f} (C_T {rc.C_T}), {worst[1]:.3f} (C_R {rc.C_R})")
    assert n > 1000
    rows = term_rows(rc.CASES["noisy_origin"], rc.expected(golden, "noisy_origin", 0)["terms"])
    assert np.array_equal(relpose(rows, through_stdin=True), relpose(rows))
    same = np.r_[rows[0, :12], rows[0, 12:24], rows[0, :12], rows[0, 12:24]]   # any two poses, on both sides
    assert not relpose(same)[0, [0, 1, 3]].any()
    bad = subprocess.run([str(relpose.exe)], input="1 2 3\n", capture_output=True, text=True)
    assert bad.returncode == 2 and "48" in bad.stderr


def test_quat_to_rot_inverts_rot_to_quat():
    rng = np.random.default_rng(11)
    Rs = [rc.rot(rng.normal(size=3), a) for a in rng.uniform(-np.pi, np.pi, size=40)]
    # Shepperd's branches: positive trace, and each diagonal entry the largest under a negative trace
    Rs += [rc.rot([0.1, 0.2, 1.0], 0.3), rc.rot([1.0, 0.05, -0.02], 3.0), rc.rot([0.03, 1.0, 0.02], 3.1), rc.rot([-0.02, 0.04, 1.0], 3.05)]
    branches = set()
    for R in Rs:
        d = np.diag(R)
        branches.add("trace" if d.sum() > 0 else int(np.argmax(d)))
        q = np.array(tum.rot_to_quat(R))
        assert np.abs(tum.quat_to_rot(q) - R).max() <= 1e-15
        assert np.abs(tum.quat_to_rot(-3.0 * q) - R).max() <= 1e-15     # sign and length of the quaternion do not matter
    assert branches == {"trace", 0, 1, 2}
    many = tum.quat_to_rot(np.array([tum.rot_to_quat(R) for R in Rs]).reshape(4, 11, 4))   # vectorised over leading axes
    assert many.shape == (4, 11, 3, 3) and np.abs(many.reshape(-1, 3, 3) - np.array(Rs)).max() <= 1e-15


def test_rpe_of_tum_files_round_trip(tmp_path):
    """write_tum -> read_tum -> quat_to_rot -> rpe: the route of a caller with two trajectory files; 9 decimals in the file bound the figures."""
    c = rc.CASES["noisy_origin"]
    tum.write_tum(tmp_path / "est.txt", c["est_t"], c["est_rot"], c["est_pos"])
    tum.write_tum(tmp_path / "gt.txt", c["gt_t"], c["gt_rot"], c["gt_pos"])
    (te, pe, qe), (tg, pg, qg) = tum.read_tum(tmp_path / "est.txt"), tum.read_tum(tmp_path / "gt.txt")
    a = tum.rpe(te, pe, tum.quat_to_rot(qe), tg, pg, tum.quat_to_rot(qg), 0.01, 0.3)
    b = tum.rpe(c["est_t"], c["est_pos"], c["est_rot"], c["gt_t"], c["gt_pos"], c["gt_rot"], 0.01, 0.3)
    assert np.array_equal(a["terms"], b["terms"]) and a["n_terms"] > 10
    for f in rc.FIGURES:
        assert abs(a[f] - b[f]) <= 2e-8, f


def test_rpe_record_is_80_bytes():
    assert C.sizeof(abi.lk_rpe) == 80 and abi.rpe_dtype().itemsize == 80
    assert [f for f, _ in abi.lk_rpe._fields_] == FIELDS == list(abi.rpe_dtype().names)


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + " %u %u %zu\\n\", sizeof(lk_rpe), "
                   + ", ".join(f"offsetof(lk_rpe, {f})" for f in FIELDS) + ", LK_RPE_INDEX, LK_RPE_NONFINITE, offsetof(lk_bucket_pose, rot)); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 80
    assert got[1:13] == [getattr(abi.lk_rpe, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76]
    assert got[1:13] == [abi.rpe_dtype().fields[f][1] for f in FIELDS]
    assert got[13:15] == [abi.LK_RPE_INDEX, abi.LK_RPE_NONFINITE] == [1, 1]
    assert got[15] == abi.bucket_pose_dtype().fields["rot"][1] == 0


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS and s in sigs
    assert len(sigs["lk_traj_rpe_dev"][1]) == 16 and len(sigs["lk_runs_rpe_dev"][1]) == 12
    assert sigs["lk_traj_rpe_dev"][1][12:15] == [C.c_double, C.c_double, C.c_uint32]
    assert callable(binding.LegKiloHip.traj_rpe_dev) and callable(binding.LegKiloHip.runs_rpe_dev)
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for phrase in ("dRe = R_i^T R_k", "atan2(s, c)", "first index in (i, n_est)", "a == b is allowed", "a step is longer than asked"):
        assert phrase in hdr, phrase   # the definition the tests implement stands in the header


def test_host_header_compiles_with_the_new_wrappers(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::runsRpeDev;\nauto b = &legkilo::KiloPath::trajRpeDev;\nint main() { return a && b ? 0 : 1; }\n')
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
