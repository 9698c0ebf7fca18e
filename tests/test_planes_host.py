"""CPU checks of the plane extraction of map clouds (lk_clouds_planes_dev / lk_clouds_planes): the case table of tests/planecloudcases.py against its
exact values through the numpy statement legkilo_amd.cloudmetrics.planes, leg-kilo_amd/csrc/lk_planes.h compiled for the host as a stand-alone
program (tools/probes/planes_host.cc: the CPU twin of the device route - the remainder compacted, the sampler, the hypotheses, the scores, the winner,
the refit in the kernel's summation order) under the address and undefined-behaviour sanitizers on every case, wrong variants of the statement that
each fail on a named case and pass elsewhere, the sampler over 10^5 counters in numpy and in the twin, the C++ wrapper, and the C-ABI: the records'
sizes and field offsets from a C program compiled against the header, the exported symbols.
The FMA variant the issue lists is not here: a decision that flips under a fused s would have to lie within 2^-53 of its threshold, which the
generator's margin of 2^-40 excludes by construction; no float32 case can be both."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import planecloudcases as pc
from legkilo_amd import abi, binding, cloudmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "planes_host.cc")
NEW_SYMBOLS = ["lk_clouds_planes_dev", "lk_clouds_planes"]
FIELDS = ["n_points", "n_on_planes", "n_rest", "n_kept", "n_planes", "status", "pad"]
PLANE_FIELDS = ["normal", "d", "centroid", "eig", "rmse", "n_inliers", "hyp"]


@pytest.fixture(scope="module")
def golden():
    return pc.golden()


def statement(c, variant=None, cloud_index=0):
    return cloudmetrics.planes(c["cloud"], c["dist"], c["n_hyp"], c["max_planes"], c["min_inliers"], c["axis"], c["cos_max_angle"], c["seed"], c["flags"], variant=variant,
                               cloud_index=cloud_index)


@pytest.fixture(scope="module")
def brute():
    """cloudmetrics.planes of every case, once."""
    return {n: statement(c) for n, c in pc.CASES.items()}


def load_generator():
    spec = importlib.util.spec_from_file_location("make_planecloud_cases", os.path.join(ROOT, "tests", "golden", "make_planecloud_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def agrees(name, golden, got):
    """every whole number of a case, exactly"""
    g = golden[name]
    return bool(np.array_equal(np.asarray(got["label"]).astype(np.int64), g["label"].astype(np.int64)) and np.array_equal(np.asarray(got["keep"]).astype(np.int64), g["keep"])
                and [int(p["n_inliers"]) for p in got["planes"]] == g["n_inliers"].tolist() and [int(p["hyp"]) for p in got["planes"]] == g["hyp"].tolist()
                and all(int(got[k]) == g[k] for k in pc.COUNTS) and int(got["n_points"]) == len(pc.CASES[name]["cloud"]))


def coefficients_hold(name, golden, got):
    en, ec = pc.coefficient_errors(pc.CASES[name]["cloud"], golden[name], got["planes"])
    return en <= pc.C_NORMAL and ec <= pc.C_COORD, (en, ec)


def test_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "leg-kilo_amd", "csrc", "lk_planes.h")).read()
    pub = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    val = lambda text, name: int(re.search(rf"#define\s+{name}\s+(\d+)u", text).group(1))   # noqa: E731
    assert (val(hdr, "LK_PLANES_GROUP"), val(hdr, "LK_PLANES_TILE"), val(hdr, "LK_PLANES_CHUNK")) == (pc.GROUP, pc.TILE, pc.CHUNK)
    assert (pc.GROUP, pc.TILE, pc.CHUNK) == (cloudmetrics.PLANES_GROUP, cloudmetrics.PLANES_TILE, cloudmetrics.PLANES_CHUNK)
    assert val(hdr, "LK_PLANES_HYP_LIMIT") == val(pub, "LK_PLANES_MAX_HYP") == abi.LK_PLANES_MAX_HYP == cloudmetrics.LK_PLANES_MAX_HYP == 4096
    assert val(pub, "LK_PLANES_MAX_PLANES") == abi.LK_PLANES_MAX_PLANES == cloudmetrics.LK_PLANES_MAX_PLANES == 16


def test_table_holds_what_the_issue_lists(golden):
    assert pc.SIZES == [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049] and pc.HYPS == [1, 63, 64, 65, 256]
    for n in pc.SIZES:
        c, g = pc.CASES[f"s{n}"], golden[f"s{n}"]
        assert len(c["cloud"]) == n and g["status"] == 0 and g["n_on_planes"] + g["n_rest"] == n and (n in (3, 4)) == (pc.params(c) != pc.MAIN)
        assert g["n_planes"] == (0 if n < 3 else 1 if n < 255 else 3), n
    assert all(max(c["n_hyp"] for c in pc.CASES.values()) <= 256 and len(c["cloud"]) <= 2049 for c in pc.CASES.values())
    for h in pc.HYPS:
        if h != pc.N_HYP:
            assert pc.CASES[f"h{h}"]["n_hyp"] == h and np.array_equal(pc.CASES[f"h{h}"]["cloud"], pc.CASES["h1"]["cloud"]) and golden[f"h{h}"]["n_planes"] >= 1
    assert golden["h63"]["hyp"].tolist() == golden["h65"]["hyp"].tolist() and golden["h256"]["hyp"].max() >= 65        # more hypotheses: a later, better one wins
    mid = pc.groups()[pc.MAIN]
    assert all(0 < mid.index(n) < len(mid) - 1 for n in ("nan_cloud", "inf_cloud", "empty_mid")) and len(pc.CASES["empty_mid"]["cloud"]) == 0
    for name, st in (("nan_cloud", 1), ("inf_cloud", 1), ("range_at", 2), ("range_below", 0)):
        g = golden[name]
        assert g["status"] == st and (not st or (g["n_on_planes"] + g["n_rest"] + g["n_kept"] + g["n_planes"] == 0 and (g["label"] == pc.NONE).all() and not g["keep"].any())), name
    assert np.abs(pc.CASES["range_at"]["cloud"]).max() == 2.0 ** 30 and np.abs(pc.CASES["range_below"]["cloud"]).max() == np.nextafter(np.float32(2.0 ** 30), np.float32(0))
    assert golden["range_below"]["n_inliers"].tolist() == [3]
    # the threshold exactly
    a, o = pc.CASES["thr_at"], pc.CASES["thr_out"]
    assert set(pc.sample(a["seed"], 0, 0, 4)) == {0, 1, 2} and a["cloud"][:3].tolist() == [[0, 0, 0], [4, 0, 0], [0, 4, 0]] and a["dist"] == 0.25 and a["n_hyp"] == 1
    assert a["cloud"][3, 2] == 0.25 and o["cloud"][3, 2] == np.nextafter(np.float32(0.25), np.float32(1)) and pc.params(a) == pc.params(o)
    assert golden["thr_at"]["label"].tolist() == [0, 0, 0, 0] and golden["thr_out"]["label"].tolist() == [0, 0, 0, pc.NONE]
    # score ties and skipped hypotheses
    c = pc.CASES["coplanar"]
    i = pc.sample(c["seed"], 0, 0, 64)
    assert not np.cross(c["cloud"][i[1]] - c["cloud"][i[0]], c["cloud"][i[2]] - c["cloud"][i[0]]).any()                  # hypothesis 0: q == 0 exactly
    assert golden["coplanar"]["hyp"].tolist() == [1] and golden["coplanar"]["n_inliers"].tolist() == [64] and golden["coplanar"]["n_planes"] == 1
    t = golden["two_planes_equal"]
    assert t["n_inliers"].tolist() == [32, 32] and t["hyp"][0] == 8 and len(set(pc.CASES["two_planes_equal"]["cloud"][t["label"] == 0][:, 2])) == 1
    assert golden["all_duplicates"]["n_planes"] == 0 and golden["on_line"]["n_planes"] == 0 and golden["on_line_plus"]["n_inliers"].tolist() == [13]
    # the axis
    fw = pc.CASES["floor_wall"]["cloud"]
    floor = fw[:, 2] == 0.0
    assert floor.sum() == 200 and (~floor).sum() == 400 and pc.CASES["floor_wall"]["axis"] == (0.0, 0.0, 1.0) and pc.CASES["floor_wall"]["cos_max_angle"] == pc.COS10
    assert np.array_equal(golden["floor_wall"]["label"] == 0, floor) and np.array_equal(golden["floor_wall_free"]["label"] == 0, ~floor)
    assert pc.CASES["floor_wall_cos0"]["cos_max_angle"] == 0.0 and pc.CASES["floor_wall_cos0"]["axis"] is not None and np.array_equal(golden["floor_wall_cos0"]["label"] == 0, ~floor)
    tl = pc.CASES["tilt_in_out"]["cloud"]
    inside = tl[:, 2] < 1.0
    assert inside.sum() == 150 and np.array_equal(golden["tilt_in_out"]["label"] == 0, inside) and np.array_equal(golden["tilt_free"]["label"] == 0, ~inside)
    assert np.rad2deg(np.arctan(1 / 8)) < 10 < np.rad2deg(np.arctan(1 / 4)) and pc.CASES["tilt_in_out"]["axis"] == (0.0, 0.0, 2.0)
    # peeling
    z = pc.CASES["peel"]["cloud"][:, 2]
    g = golden["peel"]
    assert g["n_inliers"].tolist() == [900, 500, 200] and g["n_rest"] == 100 and np.array_equal(g["label"], np.where(z == 0, 0, np.where(z == 3, 1, np.where(z == 6, 2, pc.NONE))))
    assert golden["peel_max2"]["n_inliers"].tolist() == [900, 500] and pc.CASES["peel_max2"]["max_planes"] == 2 and golden["peel_max2"]["n_rest"] == 300
    assert golden["peel_min201"]["n_inliers"].tolist() == [900, 500] and (pc.CASES["peel"]["min_inliers"], pc.CASES["peel_min201"]["min_inliers"]) == (200, 201)
    assert pc.CASES["peel_min201"]["max_planes"] == 4 and golden["peel_keep_planes"]["n_kept"] == 1600 and golden["peel"]["n_kept"] == 100
    s = golden["short_after_round"]
    assert s["label"].tolist() == [0, 0, 0, 0, pc.NONE] and s["n_planes"] == 1 and pc.CASES["short_after_round"]["max_planes"] == 3
    # independence and placement
    assert np.array_equal(pc.CASES["twin_a"]["cloud"], pc.CASES["twin_b"]["cloud"]) and pc.NAMES.index("twin_b") == pc.NAMES.index("twin_a") + 1
    po, pf = pc.CASES["place_origin"]["cloud"].astype(np.float64), pc.CASES["place_far"]["cloud"].astype(np.float64)
    assert np.array_equal(pf - po, np.tile(pc.PLACE, (len(po), 1))) and np.array_equal(golden["place_far"]["label"], golden["place_origin"]["label"])
    assert golden["place_origin"]["n_planes"] == 2 and golden["place_far"]["hyp"].tolist() == golden["place_origin"]["hyp"].tolist()
    assert all(g_["conditioned"].all() for g_ in golden.values())
    assert os.path.getsize(pc.GOLDEN) < 1 << 20


def test_golden_file_regenerates_to_the_bit():
    mod = load_generator()
    again = mod.evaluate(pc.CASES)   # (from the frozen inputs; the generator's assertions run again, the lists of tie cases among them)
    again.update(mod.inputs(pc.CASES))
    z = np.load(pc.GOLDEN)
    assert sorted(again) == sorted(z.files)
    for k in z.files:
        assert again[k].dtype == z[k].dtype and again[k].shape == z[k].shape and again[k].tobytes() == z[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    fresh = pc.build()
    assert list(fresh) == pc.NAMES
    for name, c in fresh.items():
        f = pc.CASES[name]
        assert pc.params(c) == pc.params(f), name
        a, b = c["cloud"], f["cloud"]
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name


def test_numpy_statement_agrees_with_the_table_on_every_case(golden, brute):
    worst = [0.0, 0.0]
    for name in pc.NAMES:
        assert agrees(name, golden, brute[name]), name
        ok, (en, ec) = coefficients_hold(name, golden, brute[name])
        worst = [max(worst[0], en), max(worst[1], ec)]
        assert ok, (name, en, ec)
    print(f"\nnumpy statement: normal within {worst[0]:.3f}, centroid / d / eig / rmse^2 within {worst[1]:.3f} units of 2^-53 * scale")
    assert worst[0] <= pc.NUMPY_REACHES_NORMAL and worst[1] <= pc.NUMPY_REACHES_COORD            # the figures C is 16 times of
    assert pc.C_NORMAL == 16 * pc.NUMPY_REACHES_NORMAL and pc.C_COORD == np.ceil(16 * pc.NUMPY_REACHES_COORD)


def build_probe(tmp):
    exe = tmp / "planes_host"
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), PROBE], check=True, capture_output=True, text=True)
    return exe


def run_probe(exe, tmp, names):
    """The probe over the named cases -> {name: cloudmetrics.planes's dict, with the rounds}."""
    path = tmp / "clouds.bin"
    with open(path, "wb") as f:
        for n in names:
            c = pc.CASES[n]
            ax = c["axis"] if c["axis"] is not None else (0.0, 0.0, 0.0)
            f.write(np.array([c["dist"], c["cos_max_angle"], *ax], dtype=np.float64).tobytes()
                    + np.array([len(c["cloud"]), c["n_hyp"], c["max_planes"], c["min_inliers"], c["seed"], c["flags"] | (2 if c["axis"] is not None else 0)], dtype=np.uint64).tobytes()
                    + c["cloud"].tobytes())
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), {}, 0
    for n in names:
        h = lines[at].split()
        m = int(h[1])
        assert h[0] == "cloud" and m == len(pc.CASES[n]["cloud"]), lines[at]
        at += 1
        rounds = []
        while lines[at].startswith("round"):
            rounds.append([int(v) for v in lines[at].split()[1::2]])
            at += 1
        rows = np.array([ln.split() for ln in lines[at:at + m]], dtype=np.int64).reshape(m, 2)
        at += m
        k = int(lines[at].split()[1])
        assert lines[at].split()[0] == "planes", lines[at]
        planes = []
        for ln in lines[at + 1:at + 1 + k]:
            w = ln.split()
            v = [float.fromhex(x) for x in w[2:]]
            planes.append(dict(n_inliers=int(w[0]), hyp=int(w[1]), normal=v[0:3], d=v[3], centroid=v[4:7], eig=v[7:10], rmse=v[10]))
        rec = lines[at + 1 + k].split()
        assert rec[0] == "record", rec
        out[n] = dict(status=int(h[3]), n_points=m, label=rows[:, 0], keep=rows[:, 1], planes=planes, rounds=rounds, n_planes=k, n_on_planes=int(rec[1]), n_rest=int(rec[2]),
                      n_kept=int(rec[3]))
        at += 2 + k
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("planes_probe")
    return tmp, build_probe(tmp)


def test_device_route_on_the_host_under_sanitizers(golden, probe):
    """The CPU twin on every case: clean under the sanitizers, every whole number that of the table, the coefficients within the bounds."""
    tmp, exe = probe
    got = run_probe(exe, tmp, pc.NAMES)
    worst = [0.0, 0.0]
    for name in pc.NAMES:
        assert agrees(name, golden, got[name]), name
        ok, (en, ec) = coefficients_hold(name, golden, got[name])
        worst = [max(worst[0], en), max(worst[1], ec)]
        assert ok, (name, en, ec)
    print(f"\nlk_planes.h on the host: normal within {worst[0]:.3f}, centroid / d / eig / rmse^2 within {worst[1]:.3f} units of 2^-53 * scale")
    assert [r[:2] for r in got["peel"]["rounds"]] == [[0, 1700], [1, 800], [2, 300]]          # the remainder shrinks; 100 records are below min_inliers: no round
    assert got["peel_min201"]["rounds"][2] == [2, 300, pc.NONE, 200]                                                                      # the best score is one short
    assert got["short_after_round"]["rounds"] == [[0, 5, 0, 4]]                                                                          # m = 1: no second round
    bad = subprocess.run([str(exe), str(tmp / "missing.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "cannot open" in bad.stderr
    (tmp / "short.bin").write_bytes(np.zeros(5, dtype=np.float64).tobytes() + np.array([3, 4, 1, 3, 0, 0], dtype=np.uint64).tobytes() + b"\0" * 8)
    bad = subprocess.run([str(exe), str(tmp / "short.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "truncated" in bad.stderr


WRONG = [("strict", "thr_at", "thr_out"), ("normalised", "thr_norm", "thr_at"), ("ties_last", "coplanar", "s257"), ("input_indices", "peel", "floor_wall"),
         ("samples_not_counted", "s3", "all_duplicates"), ("axis_without_aa", "tilt_in_out", "floor_wall")]


@pytest.mark.parametrize("wrong,fails_on,passes_on", WRONG)
def test_wrong_variants_of_the_statement_fail_on_a_named_case(golden, brute, wrong, fails_on, passes_on):
    assert wrong in cloudmetrics.PLANES_VARIANTS
    for name in (fails_on, passes_on):
        assert agrees(name, golden, brute[name]), "the statement without a fault agrees"
    got = statement(pc.CASES[fails_on], variant=wrong)
    assert not agrees(fails_on, golden, got)
    g = golden[fails_on]
    if wrong == "strict":                  # the point at exactly dist is left out
        assert got["label"].tolist() == [0, 0, 0, pc.NONE] and g["label"].tolist() == [0, 0, 0, 0]
    elif wrong == "normalised":            # 0.6 and 0.8 are rounded: s*s leaves 0.0625 by an ulp where 1.5625 == 1.5625 holds exactly
        assert got["label"].tolist() == [0, 0, 0, pc.NONE] and g["label"].tolist() == [0, 0, 0, 0]
    elif wrong == "ties_last":             # every valid hypothesis scores 64: the last one is taken
        assert got["planes"][0]["hyp"] > g["hyp"][0] and got["planes"][0]["n_inliers"] == 64
    elif wrong == "input_indices":         # round 0 is right, round 1 draws other records
        assert got["planes"][0]["hyp"] == g["hyp"][0] and got["planes"][0]["n_inliers"] == 900 and [p["hyp"] for p in got["planes"][1:]] != g["hyp"][1:].tolist()
    elif wrong == "samples_not_counted":   # three points: the plane through them holds nobody else
        assert got["n_planes"] == 0 and g["n_planes"] == 1
    else:                                  # the axis (0, 0, 2): g*g is four times too large and the plane at 14 degrees passes
        assert got["planes"][0]["n_inliers"] == 300 and g["n_inliers"].tolist() == [150]
    assert agrees(passes_on, golden, statement(pc.CASES[passes_on], variant=wrong)), "the fault does not show everywhere"


def test_the_cloud_index_in_the_sampler_fails_on_the_twin_clouds(golden):
    """The seventh wrong variant works on a call, not on a cloud: two clouds with the same coordinates must give the same bits."""
    names = ["twin_a", "twin_b"]
    c = pc.CASES[names[0]]
    args = (c["dist"], c["n_hyp"], c["max_planes"], c["min_inliers"], c["axis"], c["cos_max_angle"], c["seed"], c["flags"])
    right = cloudmetrics.planes_clouds([pc.CASES[n]["cloud"] for n in names], *args)
    assert all(agrees(n, golden, r) for n, r in zip(names, right)) and np.array_equal(right[0]["label"], right[1]["label"])
    wrong = cloudmetrics.planes_clouds([pc.CASES[n]["cloud"] for n in names], *args, variant="cloud_in_sampler")
    assert agrees("twin_a", golden, wrong[0]) and not agrees("twin_b", golden, wrong[1])       # cloud 0 is right: the fault does not show everywhere
    assert [p["hyp"] for p in wrong[0]["planes"]] != [p["hyp"] for p in wrong[1]["planes"]]


def test_sampler_gives_three_distinct_positions_and_is_the_twins(probe):
    tmp, exe = probe
    count = 100000
    for m in (3, 4, 5, 2 ** 16, 2 ** 32 - 1):
        for seed, r, h0 in ((0, 0, 0), (pc.SEED, 3, 17), (2 ** 64 - 5, 15, 4096 - 25000 % 4096)):
            hs = np.arange(h0, h0 + count, dtype=np.uint64)     # (counters past one round's 4096 run on into the next round's: 10^5 of them)
            idx = cloudmetrics.planes_sample(seed, r, hs, m)
            assert idx.shape == (count, 3) and (idx >= 0).all() and (idx < m).all()
            assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 0] != idx[:, 2]).all() and (idx[:, 1] != idx[:, 2]).all()
            p = subprocess.run([str(exe), "--sample", str(seed), str(r), str(h0), str(count), str(m)], capture_output=True, text=True)
            assert p.returncode == 0, p.stderr[-2000:]
            assert np.array_equal(np.array(p.stdout.split(), dtype=np.int64).reshape(count, 3), idx), (m, seed)
            for k in (0, 1, count - 1):
                assert tuple(idx[k]) == pc.sample(seed, r, h0 + k, m)                       # and the generator's, in Python integers
        if m <= 5:                                                                            # every position is drawn: nothing is out of reach
            assert set(idx.reshape(-1).tolist()) == set(range(m))


def test_records_are_64_and_96_bytes():
    assert C.sizeof(abi.lk_planes) == 64 and abi.planes_dtype().itemsize == 64 and C.sizeof(abi.lk_plane) == 96 and abi.plane_dtype().itemsize == 96
    assert [f for f, _ in abi.lk_planes._fields_] == FIELDS == list(abi.planes_dtype().names)
    assert [f for f, _ in abi.lk_plane._fields_] == PLANE_FIELDS == list(abi.plane_dtype().names)
    assert (abi.LK_PLANES_NONFINITE, abi.LK_PLANES_RANGE, abi.LK_PLANES_KEEP_PLANES, abi.LK_PLANES_NONE) == (
        cloudmetrics.LK_PLANES_NONFINITE, cloudmetrics.LK_PLANES_RANGE, cloudmetrics.LK_PLANES_KEEP_PLANES, cloudmetrics.LK_PLANES_NONE)


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu" + " %zu" * (len(FIELDS) + len(PLANE_FIELDS)) + " %u %u %u %u %u\\n\", sizeof(lk_planes), sizeof(lk_plane), "
                   + ", ".join(f"offsetof(lk_planes, {f})" for f in FIELDS) + ", " + ", ".join(f"offsetof(lk_plane, {f})" for f in PLANE_FIELDS)
                   + ", LK_PLANES_NONFINITE, LK_PLANES_RANGE, LK_PLANES_KEEP_PLANES, LK_PLANES_MAX_HYP, LK_PLANES_MAX_PLANES); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [64, 96]
    assert got[2:9] == [getattr(abi.lk_planes, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 36, 40] == [abi.planes_dtype().fields[f][1] for f in FIELDS]
    assert got[9:16] == [getattr(abi.lk_plane, f).offset for f in PLANE_FIELDS] == [0, 24, 32, 56, 80, 88, 92] == [abi.plane_dtype().fields[f][1] for f in PLANE_FIELDS]
    assert got[16:] == [abi.LK_PLANES_NONFINITE, abi.LK_PLANES_RANGE, abi.LK_PLANES_KEEP_PLANES, abi.LK_PLANES_MAX_HYP, abi.LK_PLANES_MAX_PLANES] == [1, 2, 1, 4096, 16]


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS and s in sigs and len(sigs[s][1]) == 18
        assert sigs[s][1][2:12] == [C.c_size_t, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_double, C.c_uint64, C.c_uint32]
    assert callable(binding.LegKiloHip.clouds_planes_dev) and callable(binding.LegKiloHip.clouds_planes)
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for phrase in ("s*s <= t2q", "t2q = (dist*dist) * q", "lk_planes_sample(seed, r, h, m)", "the smallest h among equal scores", "The three\n *               sample points count",
                   "m < max(3, min_inliers)", "NOT an input", "LK_PLANES_KEEP_PLANES", "LK_PLANES_RANGE", "rmse = sqrt(max(eig[0], 0))"):
        assert phrase in hdr, phrase   # the definition the tests implement stands in the header


def test_host_header_compiles_with_the_new_wrapper(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::cloudsPlanesDev;\nlegkilo::KiloPath::PlanesOut o = {};\nint main() { return a && !o.d_label ? 0 : 1; }\n')
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
