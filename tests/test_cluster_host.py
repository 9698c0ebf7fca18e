"""CPU checks of the clustering of map clouds (lk_clouds_cluster_dev / lk_clouds_cluster): the case table of tests/clustercases.py against its exact
values through the numpy statement legkilo_amd.cloudmetrics.cluster, leg-kilo_amd/csrc/lk_cluster.h compiled for the host as a stand-alone program
(tools/probes/cluster_host.cc: the CPU twin of the device route - bounds, edge rule, keys, stable sort, the walk with its three visitors, the
union-find, ids, sizes, the record) under the address and undefined-behaviour sanitizers on every case, wrong variants of the statement that each
fail on a named case and pass elsewhere, scikit-learn's DBSCAN and scipy's connected components as an independent yardstick, the C++ wrapper, and
the C-ABI: lk_cluster's size and field offsets from a C program compiled against the header, the exported symbols."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import clustercases as cc
from legkilo_amd import abi, binding, cloudmetrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
PROBE = os.path.join(ROOT, "tools", "probes", "cluster_host.cc")
NEW_SYMBOLS = ["lk_clouds_cluster_dev", "lk_clouds_cluster"]
FIELDS = ["n_points", "n_core", "n_border", "n_noise", "n_kept", "n_clusters", "n_kept_clusters", "largest", "largest_size", "status", "pad"]


@pytest.fixture(scope="module")
def golden():
    return cc.golden()


def statement(c, variant=None):
    return cloudmetrics.cluster(c["cloud"], c["reach"], c["min_pts"], c["min_size"], c["max_size"], c["flags"], variant=variant)


@pytest.fixture(scope="module")
def brute():
    """cloudmetrics.cluster of every case, once."""
    return {n: statement(c) for n, c in cc.CASES.items()}


def load_generator():
    spec = importlib.util.spec_from_file_location("make_cluster_cases", os.path.join(ROOT, "tests", "golden", "make_cluster_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cell(p, edge):
    return np.floor(np.asarray(p, dtype=np.float32).astype(np.float64) / edge).astype(np.int64)


def agrees(name, golden, got):
    """every expected value of a case, exactly"""
    g = golden[name]
    return bool(all(np.array_equal(np.asarray(got[k]).astype(np.int64), g[k].astype(np.int64)) for k in cc.PER_POINT + cc.PER_CLUSTER)
                and all(int(got[k]) == g[k] for k in cc.COUNTS) and int(got["n_points"]) == len(cc.CASES[name]["cloud"]))


def test_table_holds_what_the_issue_lists(golden):
    assert cc.SIZES == [0, 1, 2, 63, 64, 65, 255, 256, 257]
    for n in cc.SIZES:
        c, g = cc.CASES[f"s{n}"], golden[f"s{n}"]
        assert len(c["cloud"]) == n and cc.params(c) == cc.MAIN and g["status"] == 0 and g["n_core"] + g["n_border"] + g["n_noise"] == n
    assert all(golden[f"s{n}"]["n_core"] > 0 and golden[f"s{n}"]["n_border"] > 0 and golden[f"s{n}"]["n_noise"] > 0 for n in (255, 256, 257))
    assert [golden[f"s{n}"]["n_clusters"] for n in (255, 256, 257)] == [2, 1, 3]
    for name in ("chain_asc", "chain_desc", "chain_shuffled", "chain_gap_tie"):       # one cluster of all 1 000
        g = golden[name]
        assert len(cc.CASES[name]["cloud"]) == 1000 and (g["n_clusters"], g["n_core"], g["largest_size"]) == (1, 1000, 1000) and not g["label"].any(), name
    x = cc.CASES["chain_asc"]["cloud"][:, 0].astype(np.float64)
    assert (np.diff(x) < 0.25).all() and (np.diff(x) > 0.2497).all() and np.array_equal(cc.CASES["chain_desc"]["cloud"], cc.CASES["chain_asc"]["cloud"][::-1])
    assert np.array_equal(np.sort(cc.CASES["chain_shuffled"]["cloud"][:, 0]), x) and (np.diff(cc.CASES["chain_shuffled"]["cloud"][:, 0]) < 0).sum() > 400
    t, o = cc.CASES["chain_gap_tie"]["cloud"][:, 0].astype(np.float64), cc.CASES["chain_gap_out"]["cloud"][:, 0]
    assert (t[500] - t[499]) ** 2 == 0.25 * 0.25 and o[500] == np.nextafter(np.float32(o[499].astype(np.float64) + 0.25), np.float32(np.inf))
    g = golden["chain_gap_out"]
    assert g["n_clusters"] == 2 and g["cl_size"].tolist() == [500, 500] and g["cl_first"].tolist() == [0, 500]
    g = golden["many"]
    assert g["n_clusters"] == 4096 and (g["cl_size"] == 2).all() and np.array_equal(g["label"], np.repeat(np.arange(4096), 2)) and cc.CASES["many"]["min_pts"] == 2
    b, bt, nb = golden["bridge"], golden["bridge_tie"], golden["numbering"]        # the bridging point is no core point: two clusters; it joins B
    assert b["kind"].tolist() == [2] * 8 + [1] and b["label"].tolist() == [0] * 4 + [1] * 4 + [1] and b["n"][8] == 3 and b["cl_size"].tolist() == [4, 5]
    assert bt["kind"].tolist() == [2] * 8 + [1] and bt["label"].tolist() == [0] * 4 + [1] * 4 + [0] and bt["cl_first"].tolist() == [0, 4]   # the tie: core index 0, not 7
    assert nb["kind"].tolist() == [1] + [2] * 8 and nb["label"].tolist() == [1] + [0] * 4 + [1] * 4 and nb["cl_first"].tolist() == [1, 5]
    m1 = golden["mp1"]
    assert cc.CASES["mp1"]["min_pts"] == 1 and m1["n_noise"] == 0 and m1["n_border"] == 0 and m1["n_core"] == 40 and m1["n_clusters"] > 1
    assert cc.CASES["mp2"]["min_pts"] == 2 and golden["mp2"]["n_noise"] > 0
    assert cc.CASES["mp_n"]["min_pts"] == len(cc.CASES["mp_n"]["cloud"]) == 12 and (golden["mp_n"]["n_core"], golden["mp_n"]["n_clusters"]) == (12, 1)
    assert cc.CASES["mp_n1"]["min_pts"] == 13 and (golden["mp_n1"]["n_noise"], golden["mp_n1"]["n_clusters"], golden["mp_n1"]["largest_size"]) == (12, 0, 0)
    d = golden["duplicates"]
    assert d["n"].tolist() == [5, 5, 5, 5, 1, 5] and d["kind"].tolist() == [2, 2, 2, 2, 0, 2] and d["label"].tolist() == [0, 0, 0, 0, cc.NOISE, 0]
    a = golden["all_duplicates"]
    assert a["n"].tolist() == [8] * 8 and a["kind"].tolist() == [2] * 8 and a["cl_size"].tolist() == [8]
    assert len(cc.DIRECTIONS) == 26
    for d in cc.DIRECTIONS:      # the fourth point lies in the neighbour cell the name says and is linked to the query through it
        c, g = cc.CASES[cc.dir_name(d)], golden[cc.dir_name(d)]
        assert tuple(cell(c["cloud"][3], 0.25) - cell(c["cloud"][0], 0.25)) == d and g["label"].tolist() == [0, 1, 2, 0] and g["n"].tolist() == [2, 1, 1, 2]
    assert golden["two_cells_away"]["label"].tolist() == [0, 1, 2, 3] and golden["wrap_trap"]["label"].tolist() == [0, 1, 0]
    f = cc.CASES["far_clusters"]
    assert f["reach"] == 0.05 and np.linalg.norm(f["cloud"][64:].mean(0) - f["cloud"][:64].mean(0)) > 2900 and golden["far_clusters"]["n_clusters"] >= 2
    assert set(golden["far_clusters"]["label"][:64]) & set(golden["far_clusters"]["label"][64:]) <= {cc.NOISE}
    for name, st in (("nan_cloud", 1), ("inf_cloud", 1), ("range_at", 2), ("range_below", 0)):
        g = golden[name]
        assert g["status"] == st and (not st or (g["n_core"] + g["n_border"] + g["n_noise"] + g["n_clusters"] == 0 and (g["label"] == cc.NOISE).all() and not g["n"].any())), name
    assert np.abs(cc.CASES["range_at"]["cloud"]).max() / cc.CASES["range_at"]["reach"] == 2.0 ** 30 and golden["range_below"]["label"].tolist() == [0, 1, 0, 1]
    g = golden["combs"]
    assert g["n_clusters"] == 2 and g["n_noise"] == 0 and g["cl_size"].tolist() == [89, 89]
    cb = cc.CASES["combs"]["cloud"]
    ka, kb = {tuple(v) for v in cell(cb[g["label"] == 0], 0.25)}, {tuple(v) for v in cell(cb[g["label"] == 1], 0.25)}
    assert len(ka & kb) >= 20                                                         # the teeth share cells
    assert np.array_equal(cc.CASES["boundary_a"]["cloud"], cc.CASES["boundary_b"]["cloud"]) and cc.NAMES.index("boundary_b") == cc.NAMES.index("boundary_a") + 1
    sb, st_, sn, sl = (golden[n] for n in ("sf_bounds", "sf_largest_tie", "sf_largest_none", "sf_largest"))
    assert sb["cl_size"].tolist() == [3, 8, 5, 9, 8] and (cc.CASES["sf_bounds"]["min_size"], cc.CASES["sf_bounds"]["max_size"]) == (5, 8)
    assert (sb["n_kept_clusters"], sb["n_kept"]) == (3, 21) and sorted(set(sb["label"][sb["keep"] == 1])) == [1, 2, 4] and (sb["largest"], sb["largest_size"]) == (3, 9)
    assert (st_["n_kept_clusters"], st_["n_kept"]) == (1, 8) and set(st_["label"][st_["keep"] == 1]) == {1}
    assert (sn["n_kept_clusters"], sn["n_kept"], sn["n_clusters"]) == (0, 0, 5) and not sn["keep"].any()
    assert (sl["n_kept_clusters"], sl["n_kept"]) == (1, 9) and set(sl["label"][sl["keep"] == 1]) == {3}
    g = golden["contention"]
    assert len(cc.CASES["contention"]["cloud"]) == 20000 and (g["n_clusters"], g["n_core"], g["n_border"], g["largest_size"]) == (1, 19996, 4, 20000)
    assert cc.CASES["contention"]["reach"] * 0.8 == 0.25
    mid = cc.groups()[cc.MAIN]
    assert all(0 < mid.index(n) < len(mid) - 1 for n in ("nan_cloud", "inf_cloud", "empty_mid")) and len(cc.CASES["empty_mid"]["cloud"]) == 0
    assert os.path.getsize(cc.GOLDEN) < 1 << 20


def test_golden_file_regenerates_to_the_bit():
    mod = load_generator()
    again = mod.evaluate(cc.CASES)   # (from the frozen inputs; the generator's assertions run again, the lists of tie cases among them)
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
        assert cc.params(c) == cc.params(f), name
        a, b = c["cloud"], f["cloud"]
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), name
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin], b[~fin], equal_nan=True) and np.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-12), name


def test_numpy_statement_agrees_with_the_table_on_every_case(golden, brute):
    for name in cc.NAMES:
        assert agrees(name, golden, brute[name]), name


def build_probe(tmp):
    exe = tmp / "cluster_host"
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe), PROBE], check=True, capture_output=True, text=True)
    return exe


def run_probe(exe, tmp, names):
    """The probe over the named cases -> {name: cloudmetrics.cluster's dict, with the header fields and seen}."""
    path = tmp / "clouds.bin"
    with open(path, "wb") as f:
        for n in names:
            c = cc.CASES[n]
            f.write(np.array([c["reach"]], dtype=np.float64).tobytes()
                    + np.array([len(c["cloud"]), c["min_pts"], c["min_size"], c["max_size"], c["flags"]], dtype=np.uint64).tobytes() + c["cloud"].tobytes())
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines, out, at = p.stdout.split("\n"), {}, 0
    for n in names:
        h = lines[at].split()
        m = int(h[1])
        assert h[0] == "cloud" and m == len(cc.CASES[n]["cloud"]), lines[at]
        rows = np.array([ln.split() for ln in lines[at + 1:at + 1 + m]], dtype=np.int64).reshape(m, 5)
        k = int(lines[at + 1 + m].split()[1])
        assert lines[at + 1 + m].split()[0] == "clusters", lines[at + 1 + m]
        cl = np.array([ln.split() for ln in lines[at + 2 + m:at + 2 + m + k]], dtype=np.int64).reshape(k, 2)
        rec = lines[at + 2 + m + k].split()
        assert rec[0] == "record", rec
        out[n] = dict(status=int(h[3]), edge=float.fromhex(h[5]), doublings=int(h[7]), cells=[int(v) for v in h[9:12]], n_points=m, n=rows[:, 0], kind=rows[:, 1],
                      label=rows[:, 2], keep=rows[:, 3], seen=rows[:, 4], cl_size=cl[:, 0], cl_first=cl[:, 1],
                      **dict(zip(("n_core", "n_border", "n_noise", "n_kept", "n_clusters", "n_kept_clusters", "largest", "largest_size"), (int(v) for v in rec[1:]))))
        at += 3 + m + k
    return out


def seen_by_floor(cloud, edge):
    """Records in the 27 cells around each record's own, cells by floor (the record itself among them): what a walk has to look at and no more."""
    k = cell(cloud, edge)
    cells, inv, cnt = np.unique(k, axis=0, return_inverse=True, return_counts=True)
    held = {tuple(c): int(v) for c, v in zip(cells.tolist(), cnt.tolist())}
    around = np.array([sum(held.get((c[0] + a, c[1] + b, c[2] + d), 0) for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1)) for c in cells.tolist()], dtype=np.int64)
    return around[inv.reshape(-1)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cluster_probe")
    return tmp, build_probe(tmp)


def test_device_route_on_the_host_under_sanitizers(golden, probe):
    """The CPU twin on every case: clean under the sanitizers, every value that of the table, and a walk looks at exactly the records of the 27 cells."""
    tmp, exe = probe
    got = run_probe(exe, tmp, cc.NAMES)
    for name, c in cc.CASES.items():
        g = got[name]
        assert agrees(name, golden, g), name
        if not golden[name]["status"] and len(c["cloud"]):
            assert np.array_equal(g["seen"], seen_by_floor(c["cloud"], g["edge"])), name
            assert (g["doublings"] == 0) == (name != "far_clusters") and g["edge"] == c["reach"] * 2.0 ** g["doublings"], name
    far = got["far_clusters"]
    assert far["doublings"] >= 1 and np.prod(np.array(far["cells"], dtype=np.float64)) < 2.0 ** 31
    assert got["range_below"]["cells"][0] > 2 ** 29 and not got["range_at"]["n"].any()
    assert got["wrap_trap"]["cells"] == [6, 2, 1] and got["wrap_trap"]["seen"].tolist() == [2, 1, 2]   # A does not look at B, first cell of the next row
    bad = subprocess.run([str(exe), str(tmp / "missing.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "cannot open" in bad.stderr
    (tmp / "short.bin").write_bytes(np.array([0.25], dtype=np.float64).tobytes() + np.array([3, 4, 0, 9, 0], dtype=np.uint64).tobytes() + b"\0" * 8)
    bad = subprocess.run([str(exe), str(tmp / "short.bin")], capture_output=True, text=True)
    assert bad.returncode == 2 and "truncated" in bad.stderr


WRONG = [("border_links", "bridge", "chain_asc"), ("no_self", "mp_n", "mp_n1"), ("strict_reach", "chain_gap_tie", "chain_gap_out"),
         ("border_smallest_index", "bridge", "bridge_tie"), ("ids_by_member", "numbering", "bridge")]


@pytest.mark.parametrize("wrong,fails_on,passes_on", WRONG)
def test_wrong_variants_of_the_statement_fail_on_a_named_case(golden, brute, wrong, fails_on, passes_on):
    assert wrong in cloudmetrics.CLUSTER_VARIANTS
    for name in (fails_on, passes_on):
        assert agrees(name, golden, brute[name]), "the statement without a fault agrees"
    got = statement(cc.CASES[fails_on], variant=wrong)
    assert not agrees(fails_on, golden, got)
    g = golden[fails_on]
    if wrong == "border_links":            # the bridging point joins the two groups
        assert got["n_clusters"] == 1 and g["n_clusters"] == 2 and np.array_equal(got["n"], g["n"])
    elif wrong == "no_self":               # 12 points see 11 others: nobody reaches min_pts 12
        assert got["n_core"] == 0 and np.array_equal(got["n"], g["n"])
    elif wrong == "strict_reach":          # the gap at exactly the reach parts the chain
        assert got["n_clusters"] == 2 and g["n_clusters"] == 1
    elif wrong == "border_smallest_index":  # A's last point has the smaller index, B's first is nearer
        assert got["label"][8] == 0 and g["label"][8] == 1 and np.array_equal(got["kind"], g["kind"])
    else:                                  # the border point at index 0 pulls its cluster to the front
        assert got["label"].tolist() == [0] + [1] * 4 + [0] * 4 and np.array_equal(got["kind"], g["kind"])
    assert agrees(passes_on, golden, statement(cc.CASES[passes_on], variant=wrong)), "the fault does not show everywhere"


def test_links_across_clouds_fail_on_the_twin_clouds(golden):
    """The sixth wrong variant works on a call, not on a cloud: two clouds with the same coordinates taken as one."""
    names = ["boundary_a", "boundary_b"]
    c = cc.CASES[names[0]]
    args = (c["reach"], c["min_pts"], c["min_size"], c["max_size"], c["flags"])
    right = cloudmetrics.cluster_clouds([cc.CASES[n]["cloud"] for n in names], *args)
    assert all(agrees(n, golden, r) for n, r in zip(names, right))
    wrong = cloudmetrics.cluster_clouds([cc.CASES[n]["cloud"] for n in names], *args, variant="across_clouds")
    assert np.array_equal(wrong[0]["n"], 2 * golden["boundary_a"]["n"]) and not np.array_equal(wrong[0]["kind"], golden["boundary_a"]["kind"])   # every point meets its twin
    far = [cc.CASES["s65"]["cloud"], cc.CASES["s65"]["cloud"] + np.float32(8.0)]      # clouds that are nowhere near each other: the fault does not show in the labels' partition
    a, b = cloudmetrics.cluster_clouds(far, *args), cloudmetrics.cluster_clouds(far, *args, variant="across_clouds")
    assert np.array_equal(a[0]["n"], b[0]["n"]) and np.array_equal(a[0]["label"], b[0]["label"]) and np.array_equal(a[0]["kind"], b[0]["kind"])


def same_partition(a, b):
    """two labelings of the same points are equal up to renaming"""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def test_scikit_learn_and_scipy_agree_on_every_case_without_a_reach_tie(golden):
    """An independent yardstick: sklearn.cluster.DBSCAN (min_samples counts the point itself) for the core set, the noise set and the partition of the
    core points, scipy's connected components over cKDTree.query_pairs for min_pts = 1.  Only the cases the generator lists as reach ties are left
    out; which cluster a border point joins is not compared (scikit-learn takes the first core point that visits it)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    from sklearn.cluster import DBSCAN

    done = 0
    for name, c in cc.CASES.items():
        g = golden[name]
        if name in cc.REACH_TIES or g["status"] or not len(c["cloud"]):
            assert name in cc.REACH_TIES or g["status"] or name in ("s0", "empty_mid"), name
            continue
        p = c["cloud"].astype(np.float64)
        db = DBSCAN(eps=c["reach"], min_samples=c["min_pts"], algorithm="kd_tree").fit(p)
        core = np.zeros(len(p), dtype=bool)
        core[db.core_sample_indices_] = True
        assert np.array_equal(core, g["kind"] == 2), name
        assert np.array_equal(db.labels_ == -1, g["kind"] == 0), name
        assert same_partition(db.labels_[core], g["label"][core]), name
        if c["min_pts"] == 1:
            pairs = cKDTree(p).query_pairs(c["reach"], output_type="ndarray")
            graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(p), len(p)))
            k, lab = connected_components(graph, directed=False)
            assert k == g["n_clusters"] and same_partition(lab, g["label"]), name
        done += 1
    assert done == len(cc.NAMES) - len(cc.REACH_TIES) - 5    # (nan, inf, out of range, two empty clouds)


def test_n_is_the_mme_neighbourhood(brute):
    for name in ("s257", "duplicates", "chain_gap_tie", "far_clusters", "combs"):
        c = cc.CASES[name]
        n, _, _ = cloudmetrics.mme_moments(c["cloud"], c["reach"])
        assert np.array_equal(brute[name]["n"], n), name
        assert np.array_equal(cloudmetrics.sor(c["cloud"], 1, c["reach"], np.inf)["cnt"] + 1, n), name


def test_cluster_record_is_64_bytes():
    assert C.sizeof(abi.lk_cluster) == 64 and abi.cluster_dtype().itemsize == 64
    assert [f for f, _ in abi.lk_cluster._fields_] == FIELDS == list(abi.cluster_dtype().names)
    assert (abi.LK_CLUSTER_NONFINITE, abi.LK_CLUSTER_RANGE, abi.LK_CLUSTER_KEEP_LARGEST, abi.LK_CLUSTER_NOISE) == (
        cloudmetrics.LK_CLUSTER_NONFINITE, cloudmetrics.LK_CLUSTER_RANGE, cloudmetrics.LK_CLUSTER_KEEP_LARGEST, cloudmetrics.LK_CLUSTER_NOISE)
    assert (abi.LK_CLUSTER_NONFINITE, abi.LK_CLUSTER_RANGE) == (abi.LK_MME_NONFINITE, abi.LK_MME_RANGE)


def test_field_offsets_are_the_headers(tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "legkilo_hip.h"\n'
                   "int main(void) { printf(\"%zu" + " %zu" * len(FIELDS) + " %u %u %u\\n\", sizeof(lk_cluster), "
                   + ", ".join(f"offsetof(lk_cluster, {f})" for f in FIELDS) + ", LK_CLUSTER_NONFINITE, LK_CLUSTER_RANGE, LK_CLUSTER_KEEP_LARGEST); return 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 64
    assert got[1:12] == [getattr(abi.lk_cluster, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
    assert got[1:12] == [abi.cluster_dtype().fields[f][1] for f in FIELDS]
    assert got[12:15] == [abi.LK_CLUSTER_NONFINITE, abi.LK_CLUSTER_RANGE, abi.LK_CLUSTER_KEEP_LARGEST] == [1, 2, 1]


def test_symbols_are_exported_declared_and_bound():
    binding.build()
    lib = C.CDLL(binding.LIB_PATH)
    sigs = abi.signatures()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in binding.EXPORTS and s in sigs and len(sigs[s][1]) == 19
        assert sigs[s][1][2:9] == [C.c_size_t, C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    assert callable(binding.LegKiloHip.clouds_cluster_dev) and callable(binding.LegKiloHip.clouds_cluster)
    hdr = open(os.path.join(INCLUDE, "legkilo_hip.h")).read()
    assert lib.lk_abi_version() == int(re.search(r"#define\s+LK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for phrase in ("d2(i, j) <= reach * reach", "i itself counts", "n_i >= min_pts", "minimises (d2, j)", "smallest CORE member's index", "never carries a link",
                   "min_size <= size <= max_size", "LK_CLUSTER_KEEP_LARGEST", "LK_CLUSTER_RANGE"):
        assert phrase in hdr, phrase   # the definition the tests implement stands in the header


def test_host_header_compiles_with_the_new_wrapper(tmp_path):
    src = tmp_path / "wrappers.cc"
    src.write_text('#include "legkilo_host.hpp"\nauto a = &legkilo::KiloPath::cloudsClusterDev;\nlegkilo::KiloPath::ClusterOut o = {};\nint main() { return a && !o.d_label ? 0 : 1; }\n')
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "leg-kilo_amd", "host"), str(src)],
                   check=True, capture_output=True, text=True)
