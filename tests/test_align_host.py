"""CPU checks of the alignment entries (lk_clouds_align_dev / lk_clouds_align / lk_clouds_transform_dev): the case table of tests/aligncases.py
against its 50-digit values through the numpy statement legkilo_amd.cloudmetrics.align, leg-kilo_amd/csrc/lk_align.h compiled for the host as a
stand-alone program (tools/probes/align_host.cc: the CPU twin of the device route - grid search on double coordinates, the two passes of the solve
in the device's order, Horn by Jacobi, the stop decision) under the address and undefined-behaviour sanitizers on every case, five wrong variants
that each have to fail on a named case, the C++ wrappers, and the C-ABI: lk_align's size and field offsets from a C program compiled against the
header, the exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import aligncases as ac
from legkilo_amd import abi, binding, cloudmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "align_host.cc")
NEW_SYMBOLS = ["lk_clouds_align_dev", "lk_clouds_align", "lk_clouds_transform_dev"]
FIELDS = ["rot", "trans", "rmse_first", "step_rot", "step_trans", "n_matched_first", "iters", "status"]


def load_generator():
    spec = importlib.util.spec_from_file_location("make_align_cases", os.path.join(ROOT, "tests", "golden", "make_align_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return ac.golden()


@pytest.fixture(scope="module")
def gen():
    return load_generator()


@pytest.fixture(scope="module")
def restated(gen):
    """cloudmetrics.align of every case, once, in the shape aligncases.compare takes."""
    return {n: gen.run_numpy(c) for n, c in ac.CASES.items()}


def test_table_holds_what_the_issue_lists(golden):
    for nq, nr in ac.SIZES:
        c = ac.CASES[f"s{nq}_{nr}"]
        assert (len(c["query"]), len(c["ref"])) == (nq, nr)
    for name in ("s0_0", "s0_65", "s65_0", "s1_1", "s2_65"):
        g = golden[name]
        assert (g["status"], g["iters"]) == (ac.FEW, 0) and g["T"].tobytes() == ac.IDENTITY.tobytes(), name
    assert golden["s2_65"]["n_matched_first"] == 2 and golden["s1_1"]["n_matched"] == 1 and not np.isnan(golden["s1_1"]["rmse"])
    assert golden["s3_65"]["n_matched_first"] == 3 and golden["s3_65"]["iters"] >= 1 and golden["s3_65"]["status"] == ac.CONVERGED
    for name in ("s63_64", "s64_65", "s255_257", "s256_256", "s257_255", "trans", "rot_x", "rot_y", "rot_z", "both", "wide", "mirror", "partial", "guard_t0"):
        g = golden[name]
        assert g["status"] == ac.CONVERGED and g["clear"] and g["gap"] >= 0.1 and g["rmse"] < g["rmse_first"], name
    idn = golden["identity"]
    assert (idn["iters"], idn["status"]) == (1, ac.CONVERGED) and np.abs(idn["T"] - ac.IDENTITY).max() <= ac.C_R * ac.ULP * 4 and idn["rmse"] == 0.0
    assert np.array_equal(ac.CASES["identity"]["query"], ac.CASES["identity"]["ref"])
    t0 = golden["t0_answer"]
    assert t0["iters"] == 1 and ac.CASES["t0_answer"]["has_T0"] and t0["rmse_first"] < 1e-6 and 0.0 < t0["step_trans"] < 1e-8
    assert (golden["iter0"]["iters"], golden["iter0"]["status"]) == (0, 0) and golden["iter0"]["rmse"] == golden["iter0"]["rmse_first"]
    assert golden["iter0_t0"]["T"].tobytes() == ac.CASES["iter0_t0"]["T0"].tobytes() and np.isnan(golden["iter0"]["step_rot"])
    assert (golden["iter1"]["iters"], golden["iter1"]["status"]) == (1, 0) and golden["iter1"]["step_trans"] > 1e-3
    # eps 0: the pair runs to max_iter while its solves still move; a solve that repeats the one before it has both steps exactly 0, which is <= 0
    e0, e1 = golden["eps0"], golden["eps0_t0"]
    assert ac.CASES["eps0"]["eps_rot"] == ac.CASES["eps0"]["eps_trans"] == 0.0
    assert (e0["iters"], e0["status"]) == (ac.CASES["eps0"]["max_iter"], 0) and e0["step_rot"] > 0.0
    assert (e1["iters"], e1["status"], e1["step_rot"], e1["step_trans"]) == (2, ac.CONVERGED, 0.0, 0.0)
    # one call of most of the table: different counts, FEW pairs in the middle
    main = ac.groups()[(ac.M, np.asarray(ac.THR).tobytes(), ac.MAX_ITER, ac.EPS_ROT, ac.EPS_TRANS)]
    assert {golden[n]["iters"] for n in main} >= {0, 1, 2, 3} and 0 < main.index("s2_65") < main.index("wide") and len(main) >= 25
    # the same clouds at (3000, 2000, 100): R agrees, t is carried by the offset
    a, b, o = golden["far_origin"], golden["far"], np.array([3000.0, 2000.0, 100.0])
    assert np.array_equal(ac.CASES["far"]["query"].astype(np.float64), ac.CASES["far_origin"]["query"].astype(np.float64) + o)
    assert np.array_equal(ac.CASES["far"]["ref"].astype(np.float64), ac.CASES["far_origin"]["ref"].astype(np.float64) + o)
    assert (a["iters"], a["status"]) == (b["iters"], b["status"]) and np.array_equal(a["j"], b["j"])
    assert np.abs(a["T"][:9] - b["T"][:9]).max() <= 2 * ac.ULP
    assert np.abs(b["T"][9:] - (a["T"][9:] + o - a["T"][:9].reshape(3, 3) @ o)).max() <= 8 * ac.ULP * 3000.0
    m = golden["mirror"]["T"][:9].reshape(3, 3)
    assert np.linalg.det(m) > 0.999 and ac.is_rotation(m)
    mq, mr = ac.CASES["mirror"]["query"].astype(np.float64), ac.CASES["mirror"]["ref"].astype(np.float64)
    S = (mq - mq.mean(0)).T @ (mr[golden["mirror"]["j"]] - mr[golden["mirror"]["j"]].mean(0))
    assert np.linalg.det(S) < 0                                   # (the best ORTHOGONAL map of the matched pairs is a reflection)
    gd = golden["guard_t0"]
    assert gd["n_matched_first"] < 64 == gd["n_matched"] and ac.CASES["guard_t0"]["T0"][2] == 1e20 and gd["status"] == ac.CONVERGED
    z0 = ac.CASES["guard_t0"]["query"][:, 2] == 0.0
    assert np.array_equal(gd["matched_first"], z0) and 3 <= z0.sum() < 64   # the points the shear leaves where they were, and no others
    assert golden["partial"]["n_matched"] == 64 and len(ac.CASES["partial"]["query"]) == 80
    for name, st in (("nan_query", 1), ("nan_ref", 1), ("range_query", 2), ("bad_t0", ac.BAD_T0)):
        g = golden[name]
        assert (g["status"], g["iters"], g["n_matched"]) == (st, 0, 0) and np.isnan(g["rmse_first"]) and g["T"].tobytes() == ac.CASES[name]["T0"].tobytes(), name
    assert ac.CASES["plane"]["kind"] == ac.CASES["line"]["kind"] == "free" and golden["plane"]["clear"] == 1 and golden["line"]["clear"] == 0
    assert not ac.CASES["line"]["query"][:, 1:].any() and not ac.CASES["line"]["ref"][:, 1:].any()
    assert (ac.C_R, ac.C_T, ac.C_FIG) == tuple(16.0 * max(1.0, v) for v in (ac.RATIO_R, ac.RATIO_T, ac.RATIO_FIG)) and os.path.getsize(ac.GOLDEN) < 500 << 10
    assert sum(g["c2c_tie"] for g in golden.values()) >= 10


def test_golden_file_regenerates_to_the_bit(gen):
    again = gen.evaluate(ac.CASES)   # (from the frozen inputs; the generator's 50-digit assertions run again)
    again.update(gen.inputs(ac.CASES))
    z = np.load(ac.GOLDEN)
    assert sorted(again) == sorted(z.files)
    for k in z.files:
        assert again[k].dtype == z[k].dtype and again[k].shape == z[k].shape and again[k].tobytes() == z[k].tobytes(), k


def test_frozen_inputs_are_the_generators():
    fresh = ac.build()
    assert list(fresh) == ac.NAMES == ac.ORDER
    for name, c in fresh.items():
        f = ac.CASES[name]
        for k in ("max_dist", "has_T0", "max_iter", "eps_rot", "eps_trans", "kind"):
            assert c[k] == f[k], (name, k)
        assert np.array_equal(c["thr"], f["thr"]), name
        for k in ("query", "ref", "T0"):
            assert c[k].shape == f[k].shape and c[k].dtype == f[k].dtype and np.array_equal(np.isnan(c[k]), np.isnan(f[k])), (name, k)
            fin = np.isfinite(f[k])
            assert np.allclose(c[k][fin], f[k][fin], rtol=1e-6, atol=1e-12), (name, k)


def test_numpy_statement_is_exact_on_decisions_and_within_c(golden, restated):
    worst = dict(R=(0.0, None), T=(0.0, None), FIG=(0.0, None))
    for name in ac.NAMES:
        got = ac.compare(name, restated[name], golden[name])
        for k, v in got.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    print(f"cloudmetrics.align against the 50-digit values: {worst} (recorded {ac.RATIO_R}, {ac.RATIO_T}, {ac.RATIO_FIG})")
    assert worst["R"][0] <= 2.0 * ac.RATIO_R and worst["T"][0] <= 2.0 * ac.RATIO_T and worst["FIG"][0] <= 2.0 * ac.RATIO_FIG
    far = [abs(restated[n][f] - golden[n][f]) / (ac.ULP * ac.M) for n in ac.NAMES if n != "far" and golden[n]["status"] in (0, ac.CONVERGED)
           for f in ac.FIGURES if not np.isnan(golden[n][f])]
    assert max(far) < 20.0                                           # away from (3000, 2000, 100) the figures are within a few ulp of a coordinate


def test_transform_statement():
    rng = np.random.default_rng(5)
    rec = rng.uniform(-50, 50, (40, 4)).astype(np.float32)
    rec[:, 3].view(np.uint32)[:4] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0]     # NaN payloads in w
    T = ac.about(ac.rot(0, 33.0) @ ac.rot(2, -71.0), np.array([3.0, -2.0, 0.5]), np.zeros(3))
    out = cloudmetrics.transform(rec, T)
    assert out[:, 3].tobytes() == rec[:, 3].tobytes()
    want = rec[:, :3].astype(np.float64) @ T[:9].reshape(3, 3).T + T[9:]
    assert np.abs(out[:, :3] - want).max() <= 2.0 ** -24 * 128 and out.dtype == np.float32
    assert cloudmetrics.transform(rec, ac.IDENTITY).tobytes() == rec.tobytes()


def build_probe(tmp, *flags):
    exe = tmp / ("align_host" + "".join(f.replace("-D", "_") for f in flags))
    # (-fno-builtin-floor: GCC otherwise folds (long long)floor(x) into one built-in that the float-cast-overflow check does not see)
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-builtin-floor", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", *flags, "-o", str(exe), PROBE], check=True, capture_output=True, text=True)
    return exe


def write_pairs(path, names):
    with open(path, "wb") as f:
        for n in names:
            c = ac.CASES[n]
            f.write(np.array([c["max_dist"], c["eps_rot"], c["eps_trans"]], dtype=np.float64).tobytes() + c["T0"].tobytes())
            f.write(np.array([c["max_iter"], len(c["query"]), len(c["ref"])], dtype=np.uint64).tobytes())
            f.write(c["query"].tobytes() + c["ref"].tobytes())


def run_probe(exe, tmp, names):
    """The probe over the named cases -> {name: dict in the shape aligncases.compare takes (without n_within), d2}."""
    path = tmp / "pairs.bin"
    write_pairs(path, names)
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), {}, 0
    fx = float.fromhex
    for n in names:
        h = lines[at].split()
        nq = len(ac.CASES[n]["query"])
        assert h[0] == "pair" and int(h[1]) == nq, lines[at]
        t = lines[at + 1].split()
        assert t[0] == "T" and len(t) == 13
        rows = [ln.split() for ln in lines[at + 2:at + 2 + nq]]
        j = np.array([int(r[1]) for r in rows], dtype=np.uint32)
        jf = np.array([int(r[0]) for r in rows], dtype=np.uint32)
        d2 = np.array([fx(r[2]) for r in rows], dtype=np.float64)
        thr = ac.CASES[n]["thr"]
        out[n] = dict(T=np.array([fx(v) for v in t[1:]]), status=int(h[4]), iters=int(h[6]), n_matched_first=int(h[8]), rmse_first=fx(h[10]), step_rot=fx(h[12]),
                      step_trans=fx(h[14]), n_matched=int(h[16]), rmse=fx(h[18]), mean=fx(h[20]), max=fx(h[22]), worst=int(h[24]), j=j, matched=j != ac.NO_MATCH,
                      j_first=jf, matched_first=jf != ac.NO_MATCH, d2=d2, n_within=[int((d2[j != ac.NO_MATCH] <= t_ * t_).sum()) for t_ in thr])
        at += 2 + nq
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("align_probe")
    return tmp, build_probe(tmp)


def test_cpu_twin_under_sanitizers(golden, restated, probe):
    """lk_align.h's loop on every case: clean under the sanitizers, every decision the generator's, T and the figures within tolerance; the grid
    search on double coordinates gives the brute force's (j, matched) in the first and in the final search."""
    tmp, exe = probe
    got = run_probe(exe, tmp, ac.NAMES)
    worst = dict(R=0.0, T=0.0, FIG=0.0)
    for name in ac.NAMES:
        r = ac.compare(name, got[name], golden[name])
        worst = {k: max(worst[k], r[k]) for k in worst}
        if golden[name]["clear"]:
            assert np.array_equal(got[name]["j"], restated[name]["j"]) and np.array_equal(got[name]["j_first"], restated[name]["j_first"]), name
    print(f"the CPU twin against the 50-digit values: {worst}")
    bad = subprocess.run([str(exe), str(tmp / "missing.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "cannot open" in bad.stderr
    (tmp / "short.bin").write_bytes(b"\0" * (15 * 8) + np.array([1, 3, 0], dtype=np.uint64).tobytes() + b"\0" * 8)
    bad = subprocess.run([str(exe), str(tmp / "short.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "truncated" in bad.stderr


WRONG = [("compose", "far"), ("reflect", "mirror"), ("all_n", "partial"), ("one_eps", "trans")]


@pytest.mark.parametrize("variant,name", WRONG)
def test_a_wrong_restatement_fails_on_its_case(variant, name, golden, gen, restated):
    """compose: the solve from the moved points with raw moments, composed onto T - at (3000, 2000, 100) the moments lose what the centring keeps.
    reflect: SVD without the determinant fix.  all_n: the centroids divided by the query size, not by the matched count.  one_eps: the stop test
    on eps_rot alone - a pure translation has a first solve that turns by rounding only."""
    ac.compare(name, restated[name], golden[name])                   # the statement itself passes ...
    with pytest.raises(AssertionError):                              # ... the variant does not
        ac.compare(name, gen.run_numpy(ac.CASES[name], variant), golden[name])
    other = "s64_65" if variant != "compose" else "far_origin"
    if variant in ("reflect", "one_eps"):                            # ... and it is this case that tells: elsewhere the variant passes
        ac.compare(other, gen.run_numpy(ac.CASES[other], variant), golden[other])


def test_without_the_range_guard_the_sanitizers_stop_the_sheared_case(probe):
    """The fifth wrong variant, -DLK_ALIGN_NO_GUARD.  By brute force the guard changes no result, so the numpy statement cannot show it; what it
    protects is the conversion of floor(m / edge) to an integer in the grid search, which the probe's float-cast-overflow check reports for the
    points that guard_t0's T0 sends to 1e19 m.  A case whose moved points stay in range passes without the guard."""
    tmp, _ = probe
    exe = build_probe(tmp, "-DLK_ALIGN_NO_GUARD")
    write_pairs(tmp / "guard.bin", ["guard_t0"])
    p = subprocess.run([str(exe), str(tmp / "guard.bin")], capture_output=True, text=True)
    assert p.returncode != 0 and "runtime error" in p.stderr and "outside the range of representable values" in p.stderr, p.stderr[-1000:]
    assert run_probe(exe, tmp, ["s64_65"])["s64_65"]["iters"] == 2


def test_align_record_is_136_bytes():
    assert C.sizeof(abi.lk_align) == 136 and abi.align_dtype().itemsize == 136
    assert [f for f, _ in abi.lk_align._fields_] == FIELDS == list(abi.align_dtype().names)
    want = (1, 2, 4, 8, 16)
    assert (abi.LK_ALIGN_NONFINITE, abi.LK_ALIGN_RANGE, abi.LK_ALIGN_FEW, abi.LK_ALIGN_CONVERGED, abi.LK_ALIGN_BAD_T0) == want
    assert (cloudmetrics.LK_ALIGN_NONFINITE, cloudmetrics.LK_ALIGN_RANGE, cloudmetrics.LK_ALIGN_FEW, cloudmetrics.LK_ALIGN_CONVERGED, cloudmetrics.LK_ALIGN_BAD_T0) == want
    assert (ac.FEW, ac.CONVERGED, ac.BAD_T0) == want[2:]


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + " %u %u %u %u %u\\n\", sizeof(lk_align), "
                   + ", ".join(f"offsetof(lk_align, {f})" for f in FIELDS)
                   + ", LK_ALIGN_NONFINITE, LK_ALIGN_RANGE, LK_ALIGN_FEW, LK_ALIGN_CONVERGED, LK_ALIGN_BAD_T0); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 136
    assert got[1:9] == [getattr(abi.lk_align, f).offset for f in FIELDS] == [0, 72, 96, 104, 112, 120, 128, 132]
    assert got[1:9] == [abi.align_dtype().fields[f][1] for f in FIELDS]
    assert got[9:] == [1, 2, 4, 8, 16]


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in binding.EXPORTS and s in sigs, s
    for s in NEW_SYMBOLS[:2]:
        assert len(sigs[s][1]) == 22 and sigs[s][1][10:17] == [C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_double]
    assert sigs["lk_clouds_transform_dev"][1] == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    assert all(callable(getattr(binding.LegKiloHip, m)) for m in ("clouds_align_dev", "clouds_align", "clouds_transform_dev"))
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for phrase in ("m = ((R[3a] * x + R[3a+1] * y) + R[3a+2] * z) + t[a]", "never rounded to float32", "|m / max_dist| >= 2^30", "t' = rbar - R' pbar",
                   "step_rot <= eps_rot", "LK_ALIGN_BAD_T0", "rounded ONCE to float32"):
        assert phrase in hdr, phrase   # the definition the tests implement stands in the header


def test_host_header_compiles_with_the_new_wrappers(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::cloudsAlignDev;\nauto b = &legkilo::KiloPath::cloudsTransformDev;\n'
                   "int main() { return a && b ? 0 : 1; }\n")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
