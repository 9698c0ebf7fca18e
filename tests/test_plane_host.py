"""CPU checks of the point-to-plane alignment and normals entries (lk_clouds_align_plane_dev / lk_clouds_align_plane, lk_clouds_normals_dev /
lk_clouds_normals): the case tables of tests/planecases.py against their 50-digit values through the numpy statements
legkilo_amd.cloudmetrics.align_plane / normals, leg-kilo_amd/csrc/lk_align_plane.h and lk_normals.h compiled for the host as a stand-alone program
(tools/probes/align_plane_host.cc: the CPU twin of both device routes) under the address, undefined-behaviour and float-cast-overflow sanitizers on
every case, six wrong variants that each have to fail on a named case, the pinned Horn transposition, the C++ wrappers, and the C-ABI: the two
records' sizes and field offsets from a C program compiled against the header, the exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import aligncases as ac
import planecases as pc
from legkilo_amd import abi, binding, cloudmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "align_plane_host.cc")
NEW_SYMBOLS = ["lk_clouds_align_plane_dev", "lk_clouds_align_plane", "lk_clouds_normals_dev", "lk_clouds_normals"]
PL_FIELDS = ["rmse_plane_first", "rmse_plane", "n_used_first", "n_used"]
N_FIELDS = ["n_points", "n_valid", "status", "pad"]


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_plane_cases", os.path.join(ROOT, "tests", "golden", "make_plane_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return pc.golden(), pc.golden_normals()


@pytest.fixture(scope="module")
def restated(gen):
    """The numpy statements of every case, once."""
    return {n: gen.run_numpy(c) for n, c in pc.CASES.items()}, {n: gen.run_numpy_normals(c) for n, c in pc.NCASES.items()}


def test_tables_hold_what_the_issue_lists(golden):
    g, gn = golden
    size = lambda n: (len(pc.CASES[n]["query"]), len(pc.CASES[n]["ref"]))   # noqa: E731
    assert size("s0_0") == (0, 0) and size("s6_65") == (6, 65) and size("s255_257") == (255, 257) and size("s257_255") == (257, 255)
    assert (g["s0_0"]["status"], g["s0_0"]["iters"]) == (pc.FEW, 0) and np.isnan(g["s0_0"]["rmse_plane"])
    assert g["s6_65"]["n_used_first"] == 6 and g["s6_65"]["status"] == pc.CONVERGED and g["s6_65"]["iters"] >= 2           # the smallest solve
    assert (g["five_used"]["n_used"], g["five_used"]["status"], g["five_used"]["iters"]) == (5, pc.FEW, 0) and size("five_used")[0] == 5
    for name in ("s6_65", "s255_257", "s257_255", "trans", "rot_x", "rot_y", "rot_z", "both", "far", "far_origin", "third_nan", "nonunit"):
        assert g[name]["status"] == pc.CONVERGED and 2 <= g[name]["iters"] <= 4 and g[name]["rmse_plane"] < 1e-2 * g[name]["rmse_plane_first"], name
        assert g[name]["pivots"].min() >= 2.0 ** -10 and len(g[name]["pivots"]) == 6 * g[name]["iters"], name
    assert (g["identity"]["iters"], g["identity"]["status"], g["identity"]["rmse_plane"]) == (1, pc.CONVERGED, 0.0)
    assert np.array_equal(pc.CASES["identity"]["query"], pc.CASES["identity"]["ref"])
    assert pc.CASES["t0_answer"]["has_T0"] and g["t0_answer"]["iters"] == 1 and g["t0_answer"]["rmse_plane_first"] < 1e-8
    assert (g["iter0"]["iters"], g["iter0"]["status"]) == (0, 0) and g["iter0"]["rmse_plane"] == g["iter0"]["rmse_plane_first"] and np.isnan(g["iter0"]["step_rot"])
    assert (g["iter1"]["iters"], g["iter1"]["status"]) == (1, 0) and g["iter1"]["rmse_plane"] < 0.02 * g["iter1"]["rmse_plane_first"]
    assert pc.CASES["eps0"]["eps_rot"] == pc.CASES["eps0"]["eps_trans"] == 0.0 and (g["eps0"]["iters"], g["eps0"]["status"]) == (2, 0) and g["eps0"]["step_rot"] > 0.0
    # the same clouds at (3000, 2000, 100) on the 2^-12 m raster
    o = np.array([3000.0, 2000.0, 100.0])
    for k in ("query", "ref"):
        a, b = pc.CASES["far"][k].astype(np.float64), pc.CASES["far_origin"][k].astype(np.float64)
        assert np.array_equal(a, b + o) and np.array_equal(b * 4096.0, np.round(b * 4096.0))
    a, b = g["far_origin"], g["far"]
    assert (a["iters"], a["status"], a["n_used"]) == (b["iters"], b["status"], b["n_used"]) and np.array_equal(a["j"], b["j"])
    assert np.abs(a["T"][:9] - b["T"][:9]).max() <= 2 * pc.ULP and abs(a["rmse_plane"] - b["rmse_plane"]) <= 1e-20      # (at 50 digits the offset changes nothing)
    # directions the normals leave unobserved: a zero diagonal three times, a zero pivot once; T stays, no solve is taken
    for name in ("plane", "parallel", "parallel_diag", "nz0"):
        assert (g[name]["status"], g[name]["iters"]) == (pc.DEGENERATE, 0) and g[name]["T"].tobytes() == ac.IDENTITY.tobytes(), name
        assert g[name]["rmse_plane"] == g[name]["rmse_plane_first"] > 0.0 and g[name]["n_used"] >= 48, name
    assert not pc.CASES["nz0"]["normals"][:, 2].any() and len(g["plane"]["pivots"]) == len(g["parallel"]["pivots"]) == len(g["nz0"]["pivots"]) == 0
    pv = g["parallel_diag"]["pivots"]
    assert len(pv) == 5 and (pv[:4] >= 2.0 ** -10).all() and abs(pv[4]) < 1e-40 and (np.abs(pc.CASES["parallel_diag"]["normals"]).sum(axis=1) >= 1.0).all()
    nr = pc.CASES["third_nan"]["normals"]
    assert 20 <= np.isnan(nr).any(axis=1).sum() <= 23 and not np.isnan(nr).all(axis=1).any() and g["third_nan"]["n_used"] == 43 < g["third_nan"]["n_matched"] == 64
    assert (g["all_nan"]["status"], g["all_nan"]["n_used"], g["all_nan"]["n_matched"]) == (pc.FEW, 0, 64) and np.isnan(g["all_nan"]["rmse_plane"])
    assert not np.isnan(g["all_nan"]["rmse_first"])
    ln = np.linalg.norm(pc.CASES["nonunit"]["normals"].astype(np.float64), axis=1)
    assert set(np.round(np.log2(ln)).astype(int)) == {-14, 1, -1}
    for name, st in (("nan_query", 1), ("nan_ref", 1), ("range_query", 2), ("bad_t0", pc.BAD_T0)):
        assert (g[name]["status"], g[name]["iters"], g[name]["n_used"]) == (st, 0, 0) and np.isnan(g[name]["rmse_plane_first"]), name
    main = pc.groups()[(pc.M, np.asarray(pc.THR).tobytes(), pc.MAX_ITER, pc.EPS_ROT, pc.EPS_TRANS)]
    assert len(main) >= 20 and {g[n]["iters"] for n in main} >= {0, 1, 2, 3} and 0 < main.index("five_used") < main.index("both")
    # the normals table
    assert [len(pc.NCASES[n]["cloud"]) for n in ("n0", "n1", "n255", "n257")] == [0, 1, 255, 257]
    assert gn["plane"]["valid"].sum() >= 50 and (np.abs(gn["plane"]["vec"][gn["plane"]["valid"].astype(bool)] - [0, 0, 1]).max() < 1e-12)
    assert gn["tilted_50m"]["valid"].sum() >= 50 and np.abs(pc.NCASES["tilted_50m"]["cloud"]).max() > 40.0
    for name in ("edge", "corner"):
        v, d = gn[name]["valid"].astype(bool), gn[name]["dense"].astype(bool)
        assert 0 < (d & ~v).sum() < v.sum(), name                                          # near the edge the planarity falls below the threshold
    assert gn["line"]["dense"].all() and not gn["line"]["valid"].any() and not gn["line"]["w"].any()
    assert (gn["duplicates"]["w"][:12] == 0.0).all() and not gn["duplicates"]["valid"][:12].any() and gn["duplicates"]["valid"][12:].any()
    assert (gn["at_min_pts"]["n"] == 9).all() and gn["at_min_pts"]["valid"].all() and pc.NCASES["at_min_pts"]["min_pts"] == 9
    assert (gn["below_min_pts"]["n"] == 9).all() and not gn["below_min_pts"]["dense"].any() and pc.NCASES["below_min_pts"]["min_pts"] == 10
    assert np.array_equal(pc.NCASES["w_above"]["cloud"].shape, pc.NCASES["w_below"]["cloud"].shape)
    assert gn["w_above"]["valid"].all() and gn["w_below"]["dense"].all() and not gn["w_below"]["valid"].any()
    assert pc.NCASES["w_above"]["min_planarity"] < gn["w_above"]["w"].min() and gn["w_below"]["w"].max() < pc.NCASES["w_below"]["min_planarity"]
    assert int(gn["nan"]["status"][0]) == 1 and int(gn["range"]["status"][0]) == 2 and int(gn["n0"]["status"][0]) == 0 and not gn["n1"]["dense"].any()
    assert (pc.C_R, pc.C_T, pc.C_FIG, pc.C_N, pc.C_W) == tuple(16.0 * max(1.0, v) for v in (pc.RATIO_R, pc.RATIO_T, pc.RATIO_FIG, pc.RATIO_N, pc.RATIO_W))
    assert os.path.getsize(pc.GOLDEN) < 500 << 10


def test_golden_file_regenerates_to_the_bit(gen):
    again = gen.evaluate(pc.CASES, pc.NCASES)   # (from the frozen inputs; the generator's 50-digit assertions run again)
    again.update(gen.inputs(pc.CASES, pc.NCASES))
    z = np.load(pc.GOLDEN)
    assert sorted(again) == sorted(z.files)
    for k in z.files:
        assert again[k].dtype == z[k].dtype and again[k].shape == z[k].shape and again[k].tobytes() == z[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    fresh, nfresh = pc.build(), pc.build_normals()
    assert list(fresh) == pc.NAMES == pc.ORDER and list(nfresh) == pc.NNAMES == pc.NORDER
    for name, c in fresh.items():
        f = pc.CASES[name]
        for k in ("max_dist", "has_T0", "max_iter", "eps_rot", "eps_trans", "kind"):
            assert c[k] == f[k], (name, k)
        for k in ("query", "ref", "normals", "T0", "thr"):
            assert c[k].shape == f[k].shape and c[k].dtype == f[k].dtype and np.array_equal(np.isnan(c[k]), np.isnan(f[k])), (name, k)
            fin = np.isfinite(f[k])
            assert np.allclose(c[k][fin], f[k][fin], rtol=1e-6, atol=1e-12), (name, k)
    for name, c in nfresh.items():
        f = pc.NCASES[name]
        assert (c["radius"], c["min_pts"], c["min_planarity"]) == (f["radius"], f["min_pts"], f["min_planarity"]) and c["cloud"].shape == f["cloud"].shape, name
        fin = np.isfinite(f["cloud"])
        assert np.array_equal(np.isnan(c["cloud"]), np.isnan(f["cloud"])) and np.allclose(c["cloud"][fin], f["cloud"][fin], rtol=1e-6, atol=1e-12), name


def test_numpy_statements_are_exact_on_decisions_and_within_c(golden, restated):
    g, gn = golden
    ra, rn = restated
    worst = {k: (0.0, "") for k in ("R", "T", "FIG", "N", "W")}
    near = dict(R=0.0, T=0.0, FIG=0.0)
    for name in pc.NAMES:
        for k, v in pc.compare(name, ra[name], g[name]).items():
            worst[k] = max(worst[k], (v, name))
            if name != "far":
                near[k] = max(near[k], v)
    for name in pc.NNAMES:
        o = rn[name]
        for k, v in pc.compare_normals(name, o["rec"], o["n"], gn[name], o["n_valid"], o["status"]).items():
            worst[k] = max(worst[k], (v, name))
    print(f"cloudmetrics against the 50-digit values: {worst}; away from (3000, 2000, 100): {near}")
    for k, rec in (("R", pc.RATIO_R), ("T", pc.RATIO_T), ("FIG", pc.RATIO_FIG), ("N", pc.RATIO_N), ("W", pc.RATIO_W)):
        assert worst[k][0] <= 2.0 * max(rec, 0.5), (k, worst[k])
    assert near["R"] <= 3.0 and near["T"] <= 1.0 and near["FIG"] < 20.0                    # at the origin the solve is good to a few ulp


def test_horn_transposition_is_pinned():
    """lk_clouds_align_plane_dev re-orthonormalises with Horn's closed form on the TRANSPOSE: that returns a rotation as itself; the other way
    returns its inverse."""
    R = ac.rot(0, 33.0) @ ac.rot(2, -71.0) @ ac.rot(1, 12.0)
    assert np.abs(cloudmetrics.nearest_rotation(R) - R).max() <= 4 * pc.ULP
    assert np.abs(cloudmetrics.horn_rotation(R) - R.T).max() <= 4 * pc.ULP and np.abs(cloudmetrics.horn_rotation(R) - R).max() > 1.0
    bent = R + 1e-9 * np.arange(9).reshape(3, 3)                                           # a rotation up to 1e-8: the nearest one is 1e-8 away and is one
    N = cloudmetrics.nearest_rotation(bent)
    assert ac.is_rotation(N) and not ac.is_rotation(bent) and np.abs(N - R).max() < 2e-8


def build_probe(tmp, *flags):
    exe = tmp / ("align_plane_host" + "".join(f.replace("-D", "_") for f in flags))
    # (-fno-builtin-floor: GCC otherwise folds (long long)floor(x) into one built-in that the float-cast-overflow check does not see)
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-builtin-floor", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", *flags, "-o", str(exe), PROBE], check=True, capture_output=True, text=True)
    return exe


def write_pairs(path, cases):
    with open(path, "wb") as f:
        for c in cases:
            f.write(np.array([c["max_dist"], c["eps_rot"], c["eps_trans"]], dtype=np.float64).tobytes() + c["T0"].tobytes())
            f.write(np.array([c["max_iter"], len(c["query"]), len(c["ref"])], dtype=np.uint64).tobytes())
            f.write(c["query"].tobytes() + c["ref"].tobytes() + c["normals"].tobytes())


def run_align(exe, tmp, cases):
    """The probe over alignment cases -> a list of dicts in the shape planecases.compare takes."""
    path = tmp / "pairs.bin"
    write_pairs(path, cases)
    p = subprocess.run([str(exe), "align", str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), [], 0
    fx = float.fromhex
    for c in cases:
        h = lines[at].split()
        nq = len(c["query"])
        assert h[0] == "pair" and int(h[1]) == nq, lines[at]
        t = lines[at + 1].split()
        assert t[0] == "T" and len(t) == 13
        rows = [ln.split() for ln in lines[at + 2:at + 2 + nq]]
        j = np.array([int(r[1]) for r in rows], dtype=np.uint32)
        jf = np.array([int(r[0]) for r in rows], dtype=np.uint32)
        d2 = np.array([fx(r[2]) for r in rows], dtype=np.float64)
        out.append(dict(T=np.array([fx(v) for v in t[1:]]), status=int(h[4]), iters=int(h[6]), n_matched_first=int(h[8]), rmse_first=fx(h[10]), step_rot=fx(h[12]),
                        step_trans=fx(h[14]), n_matched=int(h[16]), rmse=fx(h[18]), mean=fx(h[20]), max=fx(h[22]), worst=int(h[24]), n_used_first=int(h[26]),
                        rmse_plane_first=fx(h[28]), n_used=int(h[30]), rmse_plane=fx(h[32]), j=j, matched=j != pc.NO_MATCH, j_first=jf, matched_first=jf != pc.NO_MATCH,
                        d2=d2, n_within=[int((d2[j != pc.NO_MATCH] <= t_ * t_).sum()) for t_ in c["thr"]]))
        at += 2 + nq
    return out


def run_normals(exe, tmp, cases):
    """The probe over normals cases -> a list of dicts: rec float32 [n, 4], n, n_valid, status."""
    path = tmp / "clouds.bin"
    with open(path, "wb") as f:
        for c in cases:
            f.write(np.array([c["radius"], c["min_planarity"]], dtype=np.float64).tobytes() + np.array([len(c["cloud"]), c["min_pts"]], dtype=np.uint64).tobytes())
            f.write(c["cloud"].tobytes())
    p = subprocess.run([str(exe), "normals", str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), [], 0
    for c in cases:
        h, n = lines[at].split(), len(c["cloud"])
        assert h[0] == "cloud" and int(h[1]) == n, lines[at]
        rows = [ln.split() for ln in lines[at + 1:at + 1 + n]]
        out.append(dict(rec=np.array([[float.fromhex(v) for v in r[1:]] for r in rows], dtype=np.float32).reshape(-1, 4), n=np.array([int(r[0]) for r in rows], dtype=np.uint32),
                        status=int(h[3]), n_valid=int(h[5])))
        at += 1 + n
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plane_probe")
    return tmp, build_probe(tmp)


def test_cpu_twin_under_sanitizers(golden, restated, probe):
    """lk_align_plane.h's loop and lk_normals.h on every case: clean under the sanitizers, every decision the generator's, T, the figures and the
    normals within tolerance; 1 000 solves leave R a rotation."""
    g, gn = golden
    tmp, exe = probe
    got = run_align(exe, tmp, [pc.CASES[n] for n in pc.NAMES])
    worst = dict(R=0.0, T=0.0, FIG=0.0, N=0.0, W=0.0)
    for name, o in zip(pc.NAMES, got):
        for k, v in pc.compare(name, o, g[name]).items():
            worst[k] = max(worst[k], v)
        assert np.array_equal(o["j"], restated[0][name]["j"]) and np.array_equal(o["j_first"], restated[0][name]["j_first"]), name
    gotn = run_normals(exe, tmp, [pc.NCASES[n] for n in pc.NNAMES])
    for name, o in zip(pc.NNAMES, gotn):
        for k, v in pc.compare_normals(name, o["rec"], o["n"], gn[name], o["n_valid"], o["status"]).items():
            worst[k] = max(worst[k], v)
    print(f"the CPU twin against the 50-digit values: {worst}")
    long = dict(pc.CASES["both"], max_iter=1000, eps_rot=0.0, eps_trans=0.0)
    o = run_align(exe, tmp, [long])[0]
    assert o["iters"] >= 3 and ac.is_rotation(o["T"][:9]) and o["rmse_plane"] < 1e-8
    bad = subprocess.run([str(exe), "align", str(tmp / "missing.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "cannot open" in bad.stderr
    (tmp / "short.bin").write_bytes(b"\0" * (15 * 8) + np.array([1, 3, 0], dtype=np.uint64).tobytes() + b"\0" * 8)
    for mode in ("align", "normals"):
        bad = subprocess.run([str(exe), mode, str(tmp / "short.bin")], capture_output=True, text=True)
        assert bad.returncode == 2 and "truncated" in bad.stderr, mode


WRONG = [("origin", "far", "far_origin"), ("no_scale", "nonunit", "both"), ("unit_normals", "nonunit", "both"), ("count_invalid", "third_nan", "both")]


@pytest.mark.parametrize("variant,name,other", WRONG)
def test_a_wrong_restatement_fails_on_its_case(variant, name, other, golden, gen, restated):
    """origin: the rows (and the turn) about the origin instead of mbar - at (3000, 2000, 100) the normal equations lose what the centring keeps.
    no_scale: Cholesky of H itself - normals of length 2^-14 put a pivot below 2^-20 and a well-posed pair is called degenerate.  unit_normals: the
    normals normalised - the plane residuals and the weights of the rows change.  count_invalid: the points without a plane counted into n_u."""
    g = golden[0]
    pc.compare(name, restated[0][name], g[name])                     # the statement itself passes ...
    with pytest.raises(AssertionError):                              # ... the variant does not
        pc.compare(name, gen.run_numpy(pc.CASES[name], variant), g[name])
    pc.compare(other, gen.run_numpy(pc.CASES[other], variant), g[other])   # ... and it is this case that tells: elsewhere the variant passes


def test_without_reorthonormalisation_r_drifts_over_1000_solves(gen, probe):
    """The fifth wrong variant: R1 = dR R kept as it is.  A returned R is the image of ONE unit quaternion, so R R^T - 1 is bounded by
    lk_quat_to_rot's own rounding - a dozen operations an entry, 16 ulp granted here - whatever max_iter.  Without the re-orthonormalisation the
    roundings of the products add up like a random walk: sqrt(1000) ulp after 1 000 solves.  The pair has to take them all: "far" with eps 0
    does (its residuals at 3000 m keep every step above 0; the cases at the origin repeat a solve to the bit after 5 to 7 and stop, with or
    without).  The twin built with -DLK_ALIGN_PLANE_NO_ORTHO drifts as the numpy variant does."""
    c = dict(pc.CASES["far"], max_iter=1000, eps_rot=0.0, eps_trans=0.0)
    ok, bad = gen.run_numpy(c), gen.run_numpy(c, "no_ortho")
    err = lambda T: np.abs(T[:9].reshape(3, 3) @ T[:9].reshape(3, 3).T - np.eye(3)).max() / pc.ULP   # noqa: E731
    tmp, exe = probe
    twin, twin_bad = run_align(exe, tmp, [c])[0], run_align(build_probe(tmp, "-DLK_ALIGN_PLANE_NO_ORTHO"), tmp, [c])[0]
    print(f"R R^T - 1 after 1000 solves, in ulp: numpy {err(ok['T'])}, without {err(bad['T'])}; twin {err(twin['T'])}, without {err(twin_bad['T'])}")
    assert ok["iters"] == bad["iters"] == twin["iters"] == twin_bad["iters"] == 1000
    assert ac.is_rotation(ok["T"][:9], 16.0) and ac.is_rotation(twin["T"][:9], 16.0)
    assert not ac.is_rotation(bad["T"][:9], 16.0) and not ac.is_rotation(twin_bad["T"][:9], 16.0)


def test_sign_rule_applied_after_rounding_flips_the_tied_normal(probe):
    """The sixth: the sign rule on the float32 components.  planecases.sign_tie's normal has its two large components 2.1e-8 apart in float64 and
    equal in float32; the rule on float64 makes the second positive, the rule after rounding takes the first."""
    c = pc.sign_tie()
    tmp, exe = probe
    for got in (cloudmetrics.normals(c["cloud"], c["radius"], c["min_pts"], c["min_planarity"])["rec"], run_normals(exe, tmp, [c])[0]["rec"]):
        assert (got[:, 1] > 0).all() and (got[:, 0] == -got[:, 1]).all() and (np.abs(got[:, 2]) < 1e-6).all()
    for got in (cloudmetrics.normals(c["cloud"], c["radius"], c["min_pts"], c["min_planarity"], variant="sign_f32")["rec"],
                run_normals(build_probe(tmp, "-DLK_NORMALS_SIGN_F32"), tmp, [c])[0]["rec"]):
        assert (got[:, 0] > 0).all() and (got[:, 1] < 0).all()
    k = pc.NCASES["corner"]                                           # on the table the variant changes nothing
    a, b = (cloudmetrics.normals(k["cloud"], k["radius"], k["min_pts"], k["min_planarity"], variant=v)["rec"] for v in (None, "sign_f32"))
    assert a.tobytes() == b.tobytes()


def test_rows_about_the_origin_fail_in_the_twin_too(golden, probe):
    tmp, _ = probe
    exe = build_probe(tmp, "-DLK_ALIGN_PLANE_ORIGIN")
    near, far = run_align(exe, tmp, [pc.CASES["far_origin"], pc.CASES["far"]])
    pc.compare("far_origin", near, golden[0]["far_origin"])
    with pytest.raises(AssertionError):
        pc.compare("far", far, golden[0]["far"])


def test_records_sizes_and_bits():
    assert C.sizeof(abi.lk_align_plane) == 32 == abi.align_plane_dtype().itemsize and C.sizeof(abi.lk_normals) == 24 == abi.normals_dtype().itemsize
    assert [f for f, _ in abi.lk_align_plane._fields_] == PL_FIELDS == list(abi.align_plane_dtype().names)
    assert [f for f, _ in abi.lk_normals._fields_] == N_FIELDS == list(abi.normals_dtype().names)
    assert abi.LK_ALIGN_DEGENERATE == cloudmetrics.LK_ALIGN_DEGENERATE == pc.DEGENERATE == 32 and C.sizeof(abi.lk_align) == 136


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu" + " %zu" * 8 + " %u\\n\", sizeof(lk_align_plane), sizeof(lk_normals), "
                   + ", ".join(f"offsetof(lk_align_plane, {f})" for f in PL_FIELDS) + ", " + ", ".join(f"offsetof(lk_normals, {f})" for f in N_FIELDS)
                   + ", LK_ALIGN_DEGENERATE); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [32, 24] and got[10] == 32
    assert got[2:6] == [getattr(abi.lk_align_plane, f).offset for f in PL_FIELDS] == [0, 8, 16, 24] == [abi.align_plane_dtype().fields[f][1] for f in PL_FIELDS]
    assert got[6:10] == [getattr(abi.lk_normals, f).offset for f in N_FIELDS] == [0, 8, 16, 20] == [abi.normals_dtype().fields[f][1] for f in N_FIELDS]


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in binding.EXPORTS and s in sigs, s
    for s in NEW_SYMBOLS[:2]:
        assert len(sigs[s][1]) == 24 and sigs[s][1][10:20] == [C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_double] + [C.c_void_p] * 3
    for s in NEW_SYMBOLS[2:]:
        assert sigs[s][1] == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p]
    assert all(callable(getattr(binding.LegKiloHip, m)) for m in ("clouds_align_plane_dev", "clouds_align_plane", "clouds_normals_dev", "clouds_normals"))
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    assert "Point-to-plane, scale and global (coarse) registration are not offered" not in hdr
    for phrase in ("e_i = (nx*dx + ny*dy) + nz*dz", "a_i = (c_i x n, n)", "n_u < 6: LK_ALIGN_FEW", "<= 2^-20 is LK_ALIGN_DEGENERATE", "t' = dR (t - mbar) + (mbar + v)",
                   "w = (l1 - l0) / l2", "the float64 component of largest magnitude positive", "min_pts < 3", "not normalised"):
        assert phrase in hdr, phrase   # the definitions the tests implement stand in the header


def test_host_header_compiles_with_the_new_wrappers(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::cloudsAlignPlaneDev;\nauto b = &legkilo::KiloPath::cloudsNormalsDev;\n'
                   "int main() { return a && b ? 0 : 1; }\n")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
