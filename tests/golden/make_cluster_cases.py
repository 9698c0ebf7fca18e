"""Writes tests/golden/cluster_cases.npz: the inputs of tests/clustercases.py::build() as float32 and, per case, what lk_clouds_cluster_dev has to give.

    python tests/golden/make_cluster_cases.py [path]

Decisions are taken in EXACT integer arithmetic: a float32 coordinate is an integer multiple of 2^-k, so with every coordinate of a cloud scaled by
one power of two S every d2 is a Python integer, and d2 <= reach^2 is a comparison of integers.  Which pairs are examined at all comes from a k-d
tree at reach * (1 + 2^-20): a pair it leaves out is farther than that in float64, clear of the reach by far more than the margin below.
evaluate() ASSERTS what lets the tests compare every value exactly - see tests/clustercases.py for the list - and that the cases with an exact tie
are the ones named there."""
import os
import sys
from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clustercases as cc  # noqa: E402

MARGIN = 2 ** 40


def status_of(c):
    v = c["cloud"].astype(np.float64)
    fin = np.isfinite(v)
    return (0 if fin.all() else 1) | (2 if (np.abs(v[fin] / c["reach"]) >= 2.0 ** 30).any() else 0)


def scaled_ints(cloud):
    """(P, S): the cloud as rows of Python integers, P = cloud * S exactly, S a power of two."""
    den = 1
    for v in cloud.reshape(-1):
        den = max(den, float(v).as_integer_ratio()[1])
    return [[int(Fraction(float(v)) * den) for v in row] for row in cloud], den


def evaluate_case(name, c, ties):
    cloud, r = c["cloud"], c["reach"]
    m, st = len(cloud), status_of(c)
    n = np.zeros(m, dtype=np.uint32)
    kind = np.zeros(m, dtype=np.uint8)
    label = np.full(m, cc.NOISE, dtype=np.uint32)
    keep = np.zeros(m, dtype=np.uint8)
    sizes, firsts, kept_ids = [], [], []
    if st == 0 and m:
        P, S = scaled_ints(cloud)
        r2 = Fraction(r) * Fraction(r) * S * S                 # the exact square; the rounded product differs by 2^-53, inside the margin
        r2n, r2d = r2.numerator, r2.denominator
        near = cKDTree(cloud.astype(np.float64)).query_pairs(r * (1.0 + 2.0 ** -20), output_type="ndarray")
        nb = [[] for _ in range(m)]                            # (j, d2) within reach, j != i
        for i, j in near.tolist():
            d2 = sum((a - b) ** 2 for a, b in zip(P[i], P[j]))
            lhs = d2 * r2d                                      # d2 <= r2  <=>  d2 * r2d <= r2n
            assert lhs == r2n or abs(lhs - r2n) * MARGIN >= r2n, (name, i, j, "membership neither clear nor an exact tie")
            if lhs == r2n:
                assert float(r) * float(r) == Fraction(r) * Fraction(r), (name, i, j, "an exact tie under an inexact reach * reach")
                ties["reach"].add(name)
            if lhs <= r2n:
                nb[i].append((j, d2)), nb[j].append((i, d2))
        n[:] = [1 + len(v) for v in nb]                        # the point itself counts
        core = n >= c["min_pts"]
        parent = list(range(m))

        def find(v):
            while parent[v] != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v

        for i in range(m):
            for j, _ in nb[i]:
                if j < i and core[i] and core[j]:
                    a, b = find(i), find(j)
                    parent[max(a, b)] = min(a, b)
        root = [find(i) if core[i] else -1 for i in range(m)]
        kind[core] = 2
        for i in range(m):
            if core[i]:
                continue
            cand = sorted((d2, j) for j, d2 in nb[i] if core[j])
            if not cand:
                continue
            if len(cand) > 1:
                (d0, _), (d1, _) = cand[0], cand[1]
                assert d0 == d1 or (d1 - d0) * MARGIN >= d1, (name, i, "the nearest core point is neither clear nor an exact tie")
                if d0 == d1:
                    ties["border"].add(name)
            root[i], kind[i] = root[cand[0][1]], 1
        firsts = sorted({v for v in root if v >= 0})           # a root is its component's smallest core index
        assert all(core[f] for f in firsts)
        ident = {f: k for k, f in enumerate(firsts)}
        for i in range(m):
            if root[i] >= 0:
                label[i] = ident[root[i]]
        sizes = [int((label == k).sum()) for k in range(len(firsts))]
        kept_ids = [k for k, s in enumerate(sizes) if c["min_size"] <= s <= c["max_size"]]
        if c["flags"] & cc.KEEP_LARGEST and kept_ids:
            kept_ids = [min(kept_ids, key=lambda k: (-sizes[k], k))]
        keep[np.isin(label, kept_ids)] = 1
    big = min(range(len(sizes)), key=lambda k: (-sizes[k], k)) if sizes else 0
    u32 = lambda v: np.array([v], dtype=np.uint32)              # noqa: E731
    u64 = lambda v: np.array([v], dtype=np.uint64)              # noqa: E731
    out = dict(n=n, kind=kind, label=label, keep=keep, cl_size=np.array(sizes, dtype=np.uint32), cl_first=np.array(firsts, dtype=np.uint32),
               n_core=u64(int((kind == 2).sum())), n_border=u64(int((kind == 1).sum())), n_noise=u64(0 if st else int((kind == 0).sum())), n_kept=u64(int(keep.sum())),
               n_clusters=u32(len(sizes)), n_kept_clusters=u32(len(kept_ids)), largest=u32(big), largest_size=u32(sizes[big] if sizes else 0), status=u32(st))
    return {f"{name}/out/{k_}": v for k_, v in out.items()}


def evaluate(cases):
    out, ties = {}, dict(reach=set(), border=set())
    for name, c in cases.items():
        out.update(evaluate_case(name, c, ties))
    assert sorted(ties["reach"]) == sorted(cc.REACH_TIES), ("the cases with d2 == reach^2", sorted(ties["reach"]))
    assert sorted(ties["border"]) == sorted(cc.BORDER_TIES), ("the cases with two nearest core points", sorted(ties["border"]))
    return out


def inputs(cases):
    out = {"names": np.array(list(cases))}
    for name, c in cases.items():
        out[f"{name}/in/cloud"], out[f"{name}/in/reach"] = c["cloud"], np.array([c["reach"]])
        for k in cc.PARAMS[1:]:
            out[f"{name}/in/{k}"] = np.array([c[k]], dtype=np.uint32)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "cluster_cases.npz")
    cases = cc.build()
    out = inputs(cases)
    out.update(evaluate(cases))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
