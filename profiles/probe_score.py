"""Scorer: time per rp_score_evaluate call on K = 4096 trajectories of 61 poses along the cfg3 reference path (the scene of
profiles/probe_clearance.py: feasible candidates of one cfg3 plan, evenly spread over the sampling grid, all 61 stored poses of each),
with and without RP_SCORE_EXHAUSTIVE and with and without the three per-pose outputs copied back; beside it rp_clearance_query on the
same poses, rp_score_project on 50 x 150 points (the cfg3 obstacles' positions), and the only way to ask without the library: rp_project
per pose through the binding plus the Python cost function (timed on a few trajectories, scaled to K).
C calls on caller-owned arrays, wall time around a call that ends in the library's stream synchronise; the variants alternate call by
call in one process; median, 10th and 90th percentile and minimum over the timed calls.
usage (GPU box): python profiles/probe_score.py [output file, default profiles/score_batch.txt]"""
import ctypes as C
import datetime
import math
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd")]
from commonroad_rp_amd import clearance as cl   # noqa: E402
from commonroad_rp_amd import trajectory_score as ts   # noqa: E402
from commonroad_rp_amd import workloads   # noqa: E402
from commonroad_rp_amd._capi import FLAG_MATERIALIZE_ALL, RpContext, dptr, project   # noqa: E402
from commonroad_rp_amd.cost_function import DefaultCostFunction   # noqa: E402

K, REPS, WARMUP, CHUNK, PY_TRAJ = 4096, 200, 10, 4096, 16
ip, dp, up, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
ROWS = (ts.RP_X, ts.RP_Y, ts.RP_THETA, ts.RP_V, ts.RP_A, ts.RP_KAPPA)


def cfg3_candidates():
    """(workload, rows x, y, theta, v, a, kappa [K, 61]) of K feasible candidates of one cfg3 plan, evenly spread over the grid."""
    w = workloads.cfg3(flags=FLAG_MATERIALIZE_ALL)
    ctx = RpContext(0)
    w.setup(ctx)
    ctx.plan(w.inputs)
    status, _ = ctx.fetch_status()
    feasible = np.flatnonzero(((status & 3) == 1) | ((status & 3) == 3))
    assert len(feasible) >= K, f"cfg3 has {len(feasible)} feasible candidates, fewer than {K}"
    pick = feasible[np.linspace(0, len(feasible) - 1, K).astype(np.int64)]
    n = w.inputs.params.N + 1
    rows = [np.empty((K, n)) for _ in ROWS]
    for first in range(0, len(status), CHUNK):
        sel = np.flatnonzero((pick >= first) & (pick < first + CHUNK))
        if len(sel):
            block = ctx.fetch_states(first, min(CHUNK, len(status) - first))[pick[sel] - first]
            for dst, r in zip(rows, ROWS):
                dst[sel] = block[:, r]
    ctx.close()
    assert all(np.isfinite(r).all() for r in rows)
    return w, rows, len(status), len(feasible)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "score_batch.txt")
    w, (x, y, th, v, a, ka), n_cand, n_feasible = cfg3_candidates()
    p, cost, co, n = w.inputs.params, w.inputs.cost, w.coordinate_system, x.shape[1]
    sc, q = ts.TrajectoryScorer(0), cl.ClearanceQuery(0)
    sc.set_reference(co)
    q.set_obstacles(w.obstacles)
    s, d, tcl = np.empty((K, n)), np.empty((K, n)), np.empty((K, n))
    status, cst, counts = np.empty(K, np.uint32), np.empty(K), np.zeros(8, np.int64)
    best, best_cost, n_feas = C.c_int64(), C.c_double(), C.c_int64()
    min_clear, min_pose, nearest = np.empty(K), np.empty(K, np.int32), np.empty(K, np.int32)
    fc, nb, cbest = C.c_int64(), C.c_int64(), C.c_int64()
    dyn = np.asarray(w.obstacles.dyn_obb, float)
    pts = np.resize(dyn[:, :, :2][~np.isnan(dyn[:, :, 0])], (50 * 150, 2))
    px, py = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    ps, pd, pseg, n_out = np.empty(len(px)), np.empty(len(px)), np.empty(len(px), np.int32), C.c_int64()

    def evaluate(flags, states):
        def call():
            rc = sc._lib.rp_score_evaluate(sc._h, C.byref(p), C.byref(cost), K, n, dptr(x), dptr(y), dptr(th), dptr(v), dptr(a), dptr(ka), None, flags,
                                           dptr(s) if states else None, dptr(d) if states else None, dptr(tcl) if states else None,
                                           status.ctypes.data_as(up), dptr(cst), C.byref(best), C.byref(best_cost), C.byref(n_feas),
                                           counts.ctypes.data_as(lp))
            assert rc == 0, rc
        return call

    def clearance():
        rc = q._lib.rp_clearance_query(q._h, C.byref(p), K, n, dptr(x), dptr(y), dptr(th), None, math.inf, 0.0, None, min_clear.ctypes.data_as(dp),
                                       min_pose.ctypes.data_as(ip), nearest.ctypes.data_as(ip), C.byref(fc), C.byref(nb), C.byref(cbest))
        assert rc == 0, rc

    def points():
        rc = sc._lib.rp_score_project(sc._h, len(px), dptr(px), dptr(py), dptr(ps), dptr(pd), pseg.ctypes.data_as(ip), C.byref(n_out))
        assert rc == 0, rc

    variants = [("rp_score_evaluate", evaluate(0, False)), ("rp_score_evaluate exhaustive", evaluate(ts.EXHAUSTIVE, False)),
                ("rp_score_evaluate + s, d, theta_cl", evaluate(0, True)), ("rp_score_evaluate exhaustive + s, d, theta_cl", evaluate(ts.EXHAUSTIVE, True)),
                ("rp_clearance_query cutoff inf", clearance), (f"rp_score_project {len(px)} points", points)]
    for _ in range(WARMUP):
        for _, fn in variants:
            fn()
    t = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    # pruned and exhaustive say the same, bit for bit
    variants[3][1]()
    full = [r.copy() for r in (s, d, tcl, status, cst)] + [best.value, n_feas.value]
    variants[2][1]()
    for got, want in zip([s, d, tcl, status, cst], full):
        assert np.array_equal(got.view(np.uint64 if got.dtype == np.float64 else got.dtype), want.view(np.uint64 if want.dtype == np.float64 else want.dtype))
    assert (best.value, n_feas.value) == tuple(full[5:])
    # the only way to ask without the library: rp_project per pose and the Python cost function, on PY_TRAJ trajectories
    fn_cost = DefaultCostFunction(None if math.isnan(cost.desired_speed) else cost.desired_speed, cost.desired_d,
                                  None if math.isnan(cost.desired_s) else cost.desired_s)
    fn_cost.w_a = cost.w_a
    ref_theta = co.ref_theta
    t0 = time.perf_counter()
    worst = 0.0
    for k in range(PY_TRAJ):
        sd = np.array([project(co.reference, co.ref_pos, x[k, i], y[k, i], co.proj_domain_d_limit) for i in range(n)])
        seg = np.clip(np.searchsorted(co.ref_pos, sd[:, 0], side="right") - 1, 0, len(co.ref_pos) - 2)
        lam = (sd[:, 0] - co.ref_pos[seg]) / (co.ref_pos[seg + 1] - co.ref_pos[seg])
        th_cl = (th[k] - (ref_theta[seg] + lam * (ref_theta[seg + 1] - ref_theta[seg]) ) + math.pi) % (2.0 * math.pi) - math.pi
        c_py = fn_cost.evaluate(NS(cartesian=NS(a=a[k], v=v[k]), curvilinear=NS(s=sd[:, 0], d=sd[:, 1], theta=th_cl)))
        if status[k] == 1:
            worst = max(worst, abs(c_py - cst[k]) / abs(cst[k]))
    t_py = (time.perf_counter() - t0) / PY_TRAJ
    med = {name: float(np.median(t[name])) * 1e6 for name in t}
    lines = [f"rp_score_evaluate: K = {K} trajectories of {n} poses, feasible candidates of one cfg3 plan ({n_feasible} feasible of {n_cand}), all "
             f"{n} stored poses of each, along the cfg3 reference path ({len(co.ref_pos)} vertices, {len(co.ref_pos) - 1} segments, rows in LDS: "
             f"{'yes' if len(co.ref_pos) - 1 <= 384 else 'no'})",
             f"library: {os.path.relpath(ts.LIB_PATH, REPO)}; the clearance query: {os.path.relpath(cl.LIB_PATH, REPO)}   date: {datetime.date.today().isoformat()}",
             f"wall time per C call (host copies, kernels, copy back, synchronise) over {REPS} calls after {WARMUP} warm-up calls, the variants "
             f"alternating call by call; feasible by the scorer: {n_feas.value} of {K}, reason counts {counts[1:7].tolist()}, best {best.value} "
             f"at cost {best_cost.value:.6f}; points outside the domain: {n_out.value} of {len(px)}; pruned and exhaustive outputs bit-equal",
             f"{'call':<48} {'median':>10} {'p10':>10} {'p90':>10} {'min':>10}"]
    for name, _ in variants:
        arr = np.asarray(t[name]) * 1e6
        lines.append(f"{name:<48} {np.median(arr):7.1f} us {np.percentile(arr, 10):7.1f} us {np.percentile(arr, 90):7.1f} us {arr.min():7.1f} us")
    lines += [f"exhaustive / pruned: {med['rp_score_evaluate exhaustive'] / med['rp_score_evaluate']:.2f} (no pose outputs), "
              f"{med['rp_score_evaluate exhaustive + s, d, theta_cl'] / med['rp_score_evaluate + s, d, theta_cl']:.2f} (with them); "
              f"rp_score_evaluate / rp_clearance_query: {med['rp_score_evaluate'] / med['rp_clearance_query cutoff inf']:.2f}",
              f"rp_project per pose through the binding + DefaultCostFunction.evaluate in Python: {t_py * 1e3:.2f} ms per trajectory over {PY_TRAJ} "
              f"trajectories = {t_py * K:.2f} s for {K} (no kinematic check, no selection); its costs against the library's: {worst:.1e} relative; "
              f"ratio to rp_score_evaluate: {t_py * K * 1e6 / med['rp_score_evaluate']:.0f}",
              "observations, not requirements: no threshold is set on any of these"]
    sc.close()
    q.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
