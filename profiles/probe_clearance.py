"""Clearance query: time per rp_clearance_query call on K = 4096 trajectories of 61 poses against the cfg3 obstacle tables
(commonroad_rp_amd/workloads.py: 1 static rectangle, 50 dynamic obstacles), at cutoff = inf and cutoff = 5 m, beside
rp_checker_check(RP_TRAJ_POSES) on the same inputs -- the boolean query is the floor of the work.  The trajectories are cfg3's own
candidates: one plan that keeps every state block, then 4096 kinematically feasible candidates spread evenly over the sampling grid.
C calls on caller-owned arrays, wall time around a call that ends in the library's stream synchronise; the variants alternate call
by call in one process; median, 10th and 90th percentile and minimum over the timed calls.
usage (GPU box): python profiles/probe_clearance.py [output file, default profiles/clearance_batch.txt]"""
import ctypes as C
import datetime
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd")]
from commonroad_rp_amd import clearance as cl   # noqa: E402
from commonroad_rp_amd import trajectory_check as tc   # noqa: E402
from commonroad_rp_amd import workloads   # noqa: E402
from commonroad_rp_amd._capi import FLAG_MATERIALIZE_ALL, RpContext, dptr   # noqa: E402

K, REPS, WARMUP, CHUNK = 4096, 200, 10, 4096
ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def cfg3_candidates():
    """(params, tables, x, y, theta [K, 61]) of K feasible candidates of one cfg3 plan, evenly spread over the grid."""
    w = workloads.cfg3(flags=FLAG_MATERIALIZE_ALL)
    ctx = RpContext(0)
    w.setup(ctx)
    ctx.plan(w.inputs)
    status, _ = ctx.fetch_status()
    feasible = np.flatnonzero(((status & 3) == 1) | ((status & 3) == 3))
    assert len(feasible) >= K, f"cfg3 has {len(feasible)} feasible candidates, fewer than {K}"
    pick = feasible[np.linspace(0, len(feasible) - 1, K).astype(np.int64)]
    n = w.inputs.params.N + 1
    x, y, th = np.empty((K, n)), np.empty((K, n)), np.empty((K, n))
    for first in range(0, len(status), CHUNK):
        sel = np.flatnonzero((pick >= first) & (pick < first + CHUNK))
        if len(sel):
            block = ctx.fetch_states(first, min(CHUNK, len(status) - first))
            rows = block[pick[sel] - first]
            x[sel], y[sel], th[sel] = rows[:, cl.RP_X], rows[:, cl.RP_Y], rows[:, cl.RP_THETA]
    ctx.close()
    assert np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(th).all()
    return w, x, y, th, len(status), len(feasible)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "clearance_batch.txt")
    w, x, y, th, n_cand, n_feasible = cfg3_candidates()
    p, obs, n = w.inputs.params, w.obstacles, x.shape[1]
    q, ck = cl.ClearanceQuery(0), tc.TrajectoryChecker(0)
    q.set_obstacles(obs)
    ck.set_obstacles(obs)
    min_clear, min_pose, nearest, pose_clear = np.empty(K), np.empty(K, np.int32), np.empty(K, np.int32), np.empty((K, n))
    first_pose, pose_hit = np.empty(K, np.int32), np.empty((K, n), np.uint8)
    fc, nb, best, ff, nh = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()

    def query(cutoff, per_pose):
        def call():
            rc = q._lib.rp_clearance_query(q._h, C.byref(p), K, n, dptr(x), dptr(y), dptr(th), None, cutoff, 0.0,
                                           pose_clear.ctypes.data_as(dp) if per_pose else None, min_clear.ctypes.data_as(dp),
                                           min_pose.ctypes.data_as(ip), nearest.ctypes.data_as(ip), C.byref(fc), C.byref(nb), C.byref(best))
            assert rc == 0, rc
        return call

    def check(per_pose):
        def call():
            rc = ck._lib.rp_checker_check(ck._h, C.byref(p), tc.TRAJ_POSES, K, n, dptr(x), dptr(y), dptr(th), None, first_pose.ctypes.data_as(ip),
                                          None, pose_hit.ctypes.data_as(C.POINTER(C.c_uint8)) if per_pose else None, C.byref(ff), C.byref(nh))
            assert rc == 0, rc
        return call

    variants = [("rp_clearance_query cutoff inf", query(math.inf, False)), ("rp_clearance_query cutoff 5 m", query(5.0, False)),
                ("rp_checker_check per pose", check(False)),
                ("rp_clearance_query cutoff inf + pose_clearance", query(math.inf, True)),
                ("rp_clearance_query cutoff 5 m + pose_clearance", query(5.0, True)),
                ("rp_checker_check per pose + pose_hit", check(True))]
    for _ in range(WARMUP):
        for _, fn in variants:
            fn()
    t = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, fn in variants:
            t0 = time.perf_counter()
            fn()
            t[name].append(time.perf_counter() - t0)
    # what the three calls say about the same poses: clearance 0 is the checker's hit, a cutoff changes no value at or below it
    variants[5][1]()
    variants[3][1]()
    full, n_below_inf, below5 = pose_clear.copy(), nb.value, int((min_clear <= 5.0).sum())
    assert np.array_equal(full == 0.0, pose_hit.astype(bool)) and (nb.value, fc.value) == (nh.value, ff.value)
    variants[4][1]()
    near = full <= 5.0
    assert np.array_equal(pose_clear[near], full[near]) and np.isinf(pose_clear[~near]).all()
    lines = [f"rp_clearance_query beside rp_checker_check(RP_TRAJ_POSES): K = {K} trajectories of {n} poses, feasible candidates of one cfg3 plan "
             f"({n_feasible} feasible of {n_cand}), against the cfg3 tables ({len(obs.static_obb)} static rectangle(s), {obs.dyn_obb.shape[0]} "
             f"dynamic obstacles x {obs.dyn_obb.shape[1]} steps)",
             f"library: {os.path.relpath(cl.LIB_PATH, REPO)}; the checker: {os.path.relpath(tc.LIB_PATH, REPO)}   date: {datetime.date.today().isoformat()}",
             f"wall time per C call (host copies, kernels, copy back, synchronise) over {REPS} calls after {WARMUP} warm-up calls, the variants "
             f"alternating call by call; trajectories with a hit: {n_below_inf} of {K}; with a minimum <= 5 m: {below5}; poses at 0: "
             f"{int((full == 0.0).sum())}, finite: {int(np.isfinite(full).sum())}, <= 5 m: {int(near.sum())} of {full.size}",
             f"{'call':<50} {'median':>10} {'p10':>10} {'p90':>10} {'min':>10} {'/ checker':>10}"]
    for name, _ in variants:
        a = np.asarray(t[name]) * 1e6
        floor = np.median(t["rp_checker_check per pose + pose_hit" if "pose_" in name else "rp_checker_check per pose"]) * 1e6
        lines.append(f"{name:<50} {np.median(a):7.1f} us {np.percentile(a, 10):7.1f} us {np.percentile(a, 90):7.1f} us {a.min():7.1f} us "
                     f"{np.median(a) / floor:10.2f}")
    lines.append("the ratio to the checker is an observation, not a requirement: the boolean query stops at a pose's first hit and computes no distance")
    q.close()
    ck.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
