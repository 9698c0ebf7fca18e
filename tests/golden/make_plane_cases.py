"""Writes tests/golden/plane_cases.npz: the inputs of tests/planecases.py::build() / build_normals() and, per case, what lk_clouds_align_plane_dev
and lk_clouds_normals_dev have to give - their definitions (include/legkilo_hip.h) run with mpmath at 50 digits from the float coordinates, the
float normals and the float64 T0.

    python tests/golden/make_plane_cases.py [path]

The search, its assertions (nearest against runner-up, matched against the reach, the range guard), Horn's rotation and the final search's figures
are tests/golden/make_align_cases.py's, run with this table's tolerance: a moved point may be off by dm = (3 C_R + C_T) 2^-53 L.  MARGIN = 2^10.
evaluate_case() adds
  * n_u >= 6 and `normal finite`: an integer and a bit pattern, clear once the matched flags are;
  * every Cholesky pivot of D H D, every solve: >= 2^-10, or below 10^-40 in magnitude - zero at 50 digits, where float64 gives a few 2^-53 at most,
    far below the 2^-20 of the rule; a zero diagonal entry is exactly 0 in both (a sum of squares of zeros);
  * the stop comparisons as there: step_rot MARGIN 4 C_R 2^-53 away from eps_rot, step_trans MARGIN 2 dm from eps_trans.
evaluate_ncase() asserts
  * membership of a neighbourhood: |d2 - r^2| >= MARGIN 8 2^-53 r^2 for every pair of the cloud (d2 is exact in float64 up to three roundings), so
    n_i is exact, against min_pts as well;
  * w against min_planarity: MARGIN C_W 2^-24 away;
  * the sign: the largest |component| of the normal exceeds the next by MARGIN C_N 2^-24, for every valid point."""
import importlib.util
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aligncases as ac  # noqa: E402
import planecases as pc  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_align_cases", os.path.join(HERE, "make_align_cases.py"))
mac = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mac)

mp.dps = 50
MARGIN = 2.0 ** 10
ZERO = mpf(10) ** -40


def cholesky_solve(name, what, H, g):
    """x = -D (D H D)^-1 D g at 50 digits -> (x or None, the pivots taken); the rule's decisions asserted clear."""
    dg = [H[i][i] for i in range(6)]
    if any(v <= 0 for v in dg):
        assert all(v == 0 or v >= mpf(2) ** -40 for v in dg), (name, what, "a diagonal entry is neither 0 nor clear")
        return None, []
    d = [1 / mp.sqrt(v) for v in dg]
    A = [[H[i][j] * d[i] * d[j] for j in range(6)] for i in range(6)]
    L = [[mpf(0)] * 6 for _ in range(6)]
    piv = []
    for j in range(6):
        s = A[j][j] - sum(L[j][q] * L[j][q] for q in range(j))
        assert s >= mpf(2) ** -10 or abs(s) < ZERO, (name, what, "pivot", j, float(s))
        piv.append(float(s))
        if abs(s) < ZERO:
            return None, piv
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, 6):
            L[i][j] = (A[i][j] - sum(L[i][q] * L[j][q] for q in range(j))) / L[j][j]
    y = [mpf(0)] * 6
    for i in range(6):
        y[i] = (d[i] * g[i] - sum(L[i][q] * y[q] for q in range(i))) / L[i][i]
    for i in range(5, -1, -1):
        y[i] = (y[i] - sum(L[q][i] * y[q] for q in range(i + 1, 6))) / L[i][i]
    return [-(d[i] * y[i]) for i in range(6)], piv


def quat_to_rot(w, x, y, z):
    return [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), w * w + y * y - x * x - z * z, 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), w * w + z * z - x * x - y * y]


def evaluate_case(name, c):
    q, r, nr, md = c["query"], c["ref"], c["normals"], c["max_dist"]
    n, L, st = len(q), ac.extent(c), mac.status_of(c)
    dm = (3.0 * pc.C_R + pc.C_T) * pc.ULP * L
    nan = float("nan")
    out = dict(T=c["T0"].copy(), j_first=np.full(n, ac.NO_MATCH, dtype=np.uint32), matched_first=np.zeros(n, dtype=bool), j=np.full(n, ac.NO_MATCH, dtype=np.uint32),
               matched=np.zeros(n, dtype=bool), n_within=np.zeros(len(c["thr"]), dtype=np.uint64), pivots=np.zeros(0), rmse_first=nan, step_rot=nan, step_trans=nan,
               rmse=nan, mean=nan, max=nan, gap=nan, rmse_plane_first=nan, rmse_plane=nan, iters=0, status=st, n_matched_first=0, n_matched=0, worst=0, clear=1,
               c2c_tie=0, n_used_first=0, n_used=0)
    if not st:
        fin = np.isfinite(nr.astype(np.float64)).all(axis=1) if len(nr) else np.zeros(0, dtype=bool)
        T = [mpf(float(v)) for v in c["T0"]]
        iters, stopped, first, pivots = 0, False, True, []
        while True:
            j, m, best, _ = mac.search(name, c, T, dm, f"search {iters}")
            ui = [int(i) for i in np.flatnonzero(m) if fin[j[i]]]
            P = [[mpf(float(v)) for v in q[i]] for i in ui]
            Mv = [[T[3 * a] * p[0] + T[3 * a + 1] * p[1] + T[3 * a + 2] * p[2] + T[9 + a] for a in range(3)] for p in P]
            G = [[mpf(float(v)) for v in r[j[i]]] for i in ui]
            Nn = [[mpf(float(v)) for v in nr[j[i]]] for i in ui]
            e = [sum(nn[a] * (mv[a] - g[a]) for a in range(3)) for nn, mv, g in zip(Nn, Mv, G)]
            cnt = len(ui)
            rp = float(mp.sqrt(sum(v * v for v in e) / cnt)) if cnt else nan
            if first:
                first = False
                out.update(j_first=j.copy(), matched_first=m.copy(), n_matched_first=int(m.sum()), rmse_first=float(mp.sqrt(sum(best[i] for i in np.flatnonzero(m)) / int(m.sum()))) if m.any() else nan,
                           rmse_plane_first=rp, n_used_first=cnt)
            out.update(rmse_plane=rp, n_used=cnt)
            if iters == c["max_iter"] or stopped:
                break
            if cnt < 6:
                st |= pc.FEW
                break
            mbar = [sum(v[a] for v in Mv) / cnt for a in range(3)]
            pbar = [sum(v[a] for v in P) / cnt for a in range(3)]
            rows = []
            for mv, nn in zip(Mv, Nn):
                cc = [mv[a] - mbar[a] for a in range(3)]
                rows.append([cc[1] * nn[2] - cc[2] * nn[1], cc[2] * nn[0] - cc[0] * nn[2], cc[0] * nn[1] - cc[1] * nn[0], nn[0], nn[1], nn[2]])
            H = [[sum(a[i] * a[k] for a in rows) for k in range(6)] for i in range(6)]
            g = [sum(a[i] * v for a, v in zip(rows, e)) for i in range(6)]
            x, piv = cholesky_solve(name, f"solve {iters}", H, g)
            pivots += piv
            if x is None:
                st |= pc.DEGENERATE
                break
            theta = mp.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
            dR = quat_to_rot(mpf(1), mpf(0), mpf(0), mpf(0)) if theta == 0 else quat_to_rot(mp.cos(theta / 2), *(mp.sin(theta / 2) * x[a] / theta for a in range(3)))
            R1 = [[sum(dR[3 * i + k] * T[3 * k + jj] for k in range(3)) for jj in range(3)] for i in range(3)]
            Rn, _ = mac.horn([[R1[b][a] for b in range(3)] for a in range(3)])           # (the transpose: a rotation comes back as itself)
            u = [T[9 + a] - mbar[a] for a in range(3)]
            Tn = Rn + [sum(dR[3 * a + k] * u[k] for k in range(3)) + (mbar[a] + x[3 + a]) for a in range(3)]
            E = [[Tn[3 * i] * T[3 * k] + Tn[3 * i + 1] * T[3 * k + 1] + Tn[3 * i + 2] * T[3 * k + 2] for k in range(3)] for i in range(3)]
            v = [E[2][1] - E[1][2], E[0][2] - E[2][0], E[1][0] - E[0][1]]
            s, co = mpf(0.5) * mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), mpf(0.5) * (E[0][0] + E[1][1] + E[2][2] - 1)
            step_rot = mp.atan2(s, co)
            mv_ = lambda X: [X[3 * a] * pbar[0] + X[3 * a + 1] * pbar[1] + X[3 * a + 2] * pbar[2] + X[9 + a] for a in range(3)]   # noqa: E731
            step_trans = mp.sqrt(sum((a - b) ** 2 for a, b in zip(mv_(Tn), mv_(T))))
            assert abs(step_rot - c["eps_rot"]) >= MARGIN * 4.0 * pc.C_R * pc.ULP, (name, iters, "step_rot is not clear", float(step_rot))
            assert abs(step_trans - c["eps_trans"]) >= MARGIN * 2.0 * dm, (name, iters, "step_trans is not clear", float(step_trans))
            T, iters = Tn, iters + 1
            out["step_rot"], out["step_trans"] = float(step_rot), float(step_trans)
            if step_rot <= c["eps_rot"] and step_trans <= c["eps_trans"]:
                st |= pc.CONVERGED
                stopped = True
        rmse, mean, mx, within, worst = mac.figures(name, c, m, best, dm)
        out.update(T=np.array([float(v) for v in T]) if iters else c["T0"].copy(), j=j, matched=m, n_within=np.array(within, dtype=np.uint64), rmse=rmse, mean=mean, max=mx,
                   iters=iters, status=st, n_matched=int(m.sum()), worst=worst, pivots=np.array(pivots, dtype=np.float64))
    dt = dict(T=np.float64, j_first=np.uint32, matched_first=bool, j=np.uint32, matched=bool, n_within=np.uint64, pivots=np.float64)
    res = {}
    for k in pc.OUT_ARRAYS:
        res[f"{name}/out/{k}"] = np.asarray(out[k], dtype=dt[k])
    for k in pc.OUT_FLOATS:
        res[f"{name}/out/{k}"] = np.array([out[k]], dtype=np.float64)
    for k in pc.OUT_INTS:
        res[f"{name}/out/{k}"] = np.array([out[k]], dtype=np.int64)
    return res


def evaluate_ncase(name, c):
    p, rad = c["cloud"].astype(np.float64), c["radius"]
    m = len(p)
    v = c["cloud"].astype(np.float64)
    finite = np.isfinite(v)
    st = (0 if finite.all() else 1) | (2 if (np.abs(v[finite] / rad) >= 2.0 ** 30).any() else 0)
    n, w, valid, dense, vec = np.zeros(m, dtype=np.uint32), np.full(m, np.nan), np.zeros(m, dtype=bool), np.zeros(m, dtype=bool), np.full((m, 3), np.nan)
    if not st and m:
        d = p[:, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r2 = rad * rad
        assert (np.abs(d2 - r2) >= MARGIN * 8.0 * pc.ULP * r2).all(), (name, "a neighbour at the radius")
        inside = d2 <= r2
        n = inside.sum(axis=1).astype(np.uint32)
        dense = n >= c["min_pts"]
        for i in np.flatnonzero(dense):
            U = [[mpf(float(p[k][a])) - mpf(float(p[i][a])) for a in range(3)] for k in np.flatnonzero(inside[i])]
            cnt = len(U)
            s = [sum(u[a] for u in U) for a in range(3)]
            C = mp.matrix(3, 3)
            for a in range(3):
                for b in range(3):
                    C[a, b] = (sum(u[a] * u[b] for u in U) - s[a] * s[b] / cnt) / (cnt - 1)
            E, Q = mp.eigsy(C)
            order = sorted(range(3), key=lambda k: E[k])
            l0, l1, l2 = (E[k] for k in order)
            wi = (l1 - l0) / l2 if l2 > ZERO else mpf(0)
            w[i] = float(wi)
            assert abs(wi - c["min_planarity"]) >= MARGIN * pc.C_W * pc.ULP32, (name, int(i), "w against min_planarity", float(wi))
            valid[i] = wi >= c["min_planarity"]
            if valid[i]:
                nv = [Q[a, order[0]] for a in range(3)]
                mag = sorted((abs(x) for x in nv), reverse=True)
                assert mag[0] - mag[1] >= MARGIN * pc.C_N * pc.ULP32, (name, int(i), "the sign component", float(mag[0]), float(mag[1]))
                lead = max(range(3), key=lambda a: abs(nv[a]))
                sg = -1 if nv[lead] < 0 else 1
                vec[i] = [float(sg * x) for x in nv]
    return {f"N/{name}/out/n": n, f"N/{name}/out/w": w, f"N/{name}/out/valid": valid, f"N/{name}/out/dense": dense, f"N/{name}/out/vec": vec,
            f"N/{name}/out/status": np.array([st], dtype=np.int64)}


def evaluate(cases, ncases):
    out = {}
    for name, c in cases.items():
        out.update(evaluate_case(name, c))
    for name, c in ncases.items():
        out.update(evaluate_ncase(name, c))
    return out


def inputs(cases, ncases):
    out = {"names": np.array(list(cases)), "nnames": np.array(list(ncases))}
    for name, c in cases.items():
        for k in ("query", "ref", "normals", "thr", "T0"):
            out[f"{name}/in/{k}"] = c[k]
        for k, dt in (("max_dist", np.float64), ("eps_rot", np.float64), ("eps_trans", np.float64), ("max_iter", np.int64), ("has_T0", bool)):
            out[f"{name}/in/{k}"] = np.array([c[k]], dtype=dt)
        out[f"{name}/in/kind"] = np.array([c["kind"]])
    for name, c in ncases.items():
        out[f"N/{name}/in/cloud"] = c["cloud"]
        for k, dt in (("radius", np.float64), ("min_planarity", np.float64), ("min_pts", np.int64)):
            out[f"N/{name}/in/{k}"] = np.array([c[k]], dtype=dt)
    return out


def golden_of(ev, name):
    g = {k: ev[f"{name}/out/{k}"] for k in pc.OUT_ARRAYS}
    g.update({k: float(ev[f"{name}/out/{k}"][0]) for k in pc.OUT_FLOATS})
    g.update({k: int(ev[f"{name}/out/{k}"][0]) for k in pc.OUT_INTS})
    return g


def ngolden_of(ev, name):
    return {k: ev[f"N/{name}/out/{k}"] for k in pc.N_OUT}


def run_numpy(c, variant=None):
    """legkilo_amd.cloudmetrics.align_plane of one case in the shape planecases.compare takes."""
    from legkilo_amd import cloudmetrics

    a = cloudmetrics.align_plane(c["query"], c["ref"], c["normals"], c["max_dist"], c["T0"] if c["has_T0"] else None, c["max_iter"], c["eps_rot"], c["eps_trans"],
                                 c["thr"], variant=variant)
    f = a["c2c"]
    return dict(T=a["T"], iters=a["iters"], status=a["status"], n_matched_first=a["n_matched_first"], rmse_first=a["rmse_first"], step_rot=a["step_rot"],
                step_trans=a["step_trans"], rmse=f["rmse"], mean=f["mean"], max=f["max"], n_matched=f["n_matched"], n_within=f["n_within"], worst=f["worst"],
                j_first=a["first"][0], matched_first=a["first"][1], j=f["j"], matched=f["matched"], rmse_plane_first=a["rmse_plane_first"], rmse_plane=a["rmse_plane"],
                n_used_first=a["n_used_first"], n_used=a["n_used"])


def run_numpy_normals(c, variant=None):
    from legkilo_amd import cloudmetrics

    return cloudmetrics.normals(c["cloud"], c["radius"], c["min_pts"], c["min_planarity"], variant=variant)


def numpy_ratios(cases, ncases, ev):
    """Worst ratios of the numpy statements over the tables, with where: {"R": (ratio, case), ...}; their decisions are asserted."""
    worst = {k: (0.0, None) for k in ("R", "T", "FIG", "N", "W")}
    for name, c in cases.items():
        for k, v in pc.compare(name, run_numpy(c), golden_of(ev, name), c).items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    for name, c in ncases.items():
        o = run_numpy_normals(c)
        for k, v in pc.compare_normals(name, o["rec"], o["n"], ngolden_of(ev, name), o["n_valid"], o["status"]).items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import lk_pkg  # noqa: E402

    lk_pkg.load()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plane_cases.npz")
    cases, ncases = pc.build(), pc.build_normals()
    out = inputs(cases, ncases)
    ev = evaluate(cases, ncases)
    for name in cases:
        g = golden_of(ev, name)
        print(f"{name:14s} iters {g['iters']:2d} status {g['status']:2d} matched {g['n_matched_first']:3d} -> {g['n_matched']:3d} used {g['n_used_first']:3d} -> {g['n_used']:3d} "
              f"plane {g['rmse_plane_first']:.3e} -> {g['rmse_plane']:.3e} min pivot {g['pivots'].min() if len(g['pivots']) else float('nan'):.3e}")
    for name in ncases:
        g = ngolden_of(ev, name)
        print(f"N {name:14s} points {len(g['n']):3d} dense {int(g['dense'].sum()):3d} valid {int(g['valid'].sum()):3d} status {int(g['status'][0])}")
    for k, (ratio, where) in numpy_ratios(cases, ncases, ev).items():
        print(f"numpy restatement: RATIO_{k} {ratio:.3f} at {where}")
    out.update(ev)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
