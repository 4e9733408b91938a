"""Pick: time of one rp_pick_select call on K = 64, 1 024 and 16 384 trajectories of 31 poses along the cfg2_ref_draw path (the 64 stored
trajectories of tests/golden/cfg2_ref_draw.npz, rows s, d and their derivatives over each one's own length, repeated to K, as in
profiles/lift_batch.txt) against that fixture's five dynamic obstacles, per-pose test --
  (a) with NULL planes: status, cost, the scalars and the winner's block come back, no pose plane leaves the device;
  (b) with all eight planes;
  (c) the chain it replaces, in the same process and alternating with (a) call by call: rp_lift_evaluate with all eight planes, the
      default cost in NumPy over the feasible trajectories, argsort, the poses gathered in cost order, rp_checker_check on them,
      first_free mapped back to the caller's index.
(a), (b) and (c) must name the same winner; the run fails otherwise.
C calls on caller-owned arrays, wall time around a call that ends in the library's stream synchronise; warm-up calls first, then median,
10th and 90th percentile and minimum over the timed calls.  THE CLAIM: (a) is faster than (c) at K = 1 024 and K = 16 384, which holds at
a size when (a)'s p90 is below (c)'s p10; K = 64 is launch-bound on both sides and only reported.
The GPU step is a child process under its own time limit; nothing is tried twice.  Fails without a GPU.
usage (GPU box): python profiles/probe_pick.py [output file, default profiles/pick_batch.txt]"""
import ctypes as C
import datetime
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd")]

KS, N_POSES, REPS, WARMUP = (64, 1024, 16384), 31, 100, 10
STEP_LIMIT_S = 400
FIXTURE = os.path.join(REPO, "tests", "golden", "cfg2_ref_draw.npz")


def _fixture():
    from commonroad_rp_amd._capi import make_cost, make_params
    from commonroad_rp_amd.collision import ObstacleTables
    z = dict(np.load(FIXTURE))
    veh = z["vehicle"]
    p = make_params(dt=float(z["dt"]), N=int(z["N"]), factor=int(z["factor"]), time_step0=int(z["time_step0"]), low_vel_mode=bool(z["low_vel_mode"]),
                    lon_mode=int(z["lon_mode"]), constraint_mask=int(z["constraint_mask"]), x0_lon=z["x0_lon"], x0_lat=z["x0_lat"],
                    x0_orientation=float(z["x0_orientation"]), wheelbase=veh[0], wb_rear_axle=veh[1], length=veh[2], width=veh[3], a_max=veh[4],
                    v_switch=veh[5], delta_max=veh[6], v_delta_max=veh[7])
    ds, dss = float(z["desired_speed"]), float(z["desired_s"])
    cost = make_cost(kind=int(z["cost_kind"]), w_a=float(z["w_a"]), desired_speed=None if np.isnan(ds) else ds, desired_d=float(z["desired_d"]),
                     desired_s=None if np.isnan(dss) else dss)
    obs = ObstacleTables(static_obb=z["static_obb"], static_tri=z["static_tri"], static_circ=z["static_circ"], dyn_obb=z["dyn_obb"], dyn_t0=int(z["dyn_t0"]))
    t_index = z["state_index"] // (len(z["L"]) * len(z["D"]))
    assert z["states"].shape[2] == N_POSES and z["dyn_obb"].shape[0] == 5
    return z, p, cost, obs, t_index


def _stats(samples):
    a = np.asarray(samples) * 1e6
    return [float(np.median(a)), float(np.percentile(a, 10)), float(np.percentile(a, 90)), float(a.min())]


def _clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def _default_cost(cost, lens, s, d, v, a, theta_cl):
    """DefaultCostFunction over each row's own length (cost_function.py:51-71), for all rows at once"""
    n = s.shape[1]
    valid = np.arange(n)[None, :] < lens[:, None]
    last, mid = (lens - 1)[:, None], (lens // 2)[:, None]
    at = lambda q, i: np.take_along_axis(q, i, 1)[:, 0]   # noqa: E731
    total = np.where(valid, (cost.w_a * a) ** 2, 0.0).sum(1)
    if not np.isnan(cost.desired_speed):
        total += np.where(valid, (5 * (v - cost.desired_speed)) ** 2, 0.0).sum(1) + 50 * (at(v, last) - cost.desired_speed) ** 2 + \
            100 * (at(v, mid) - cost.desired_speed) ** 2
    if not np.isnan(cost.desired_s):
        total += np.where(valid, (0.25 * (cost.desired_s - s)) ** 2, 0.0).sum(1) + (20 * (cost.desired_s - at(s, last))) ** 2
    total += np.where(valid, (0.25 * (cost.desired_d - d)) ** 2, 0.0).sum(1) + (20 * (cost.desired_d - at(d, last))) ** 2
    total += np.where(valid, (0.25 * np.abs(theta_cl)) ** 2, 0.0).sum(1) + (5 * np.abs(at(theta_cl, last))) ** 2
    return total


def step_pick():
    from commonroad_rp_amd import TrajectoryChecker, TrajectoryLifter, TrajectoryPicker
    from commonroad_rp_amd._capi import dptr
    from commonroad_rp_amd.pick import RpPickResult
    z, p, cost, obs, t_index = _fixture()
    lens64 = z["traj_len"][t_index].astype(np.int32)
    up, lp, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    tables = (z["ref_path"], z["ref_pos"], z["ref_theta"], z["ref_curv"], z["ref_curv_d"], float(z["proj_d_limit"]))
    res = {}
    with TrajectoryPicker(0) as pk, TrajectoryLifter(0) as lf, TrajectoryChecker(0) as ck:
        pk.set_reference(*tables)
        pk.set_obstacles(obs)
        lf.set_reference(*tables)
        ck.set_obstacles(obs)
        for K in KS:
            planes = [np.ascontiguousarray(np.tile(z["states"][:, r], (K // 64, 1))) for r in (7, 10, 11, 8, 12, 13)]
            lens = np.ascontiguousarray(np.tile(lens64, K // 64))
            outs = [np.empty((K, N_POSES)) for _ in range(8)]
            status, costs, block, result = np.empty(K, np.uint32), np.empty(K), np.empty((14, N_POSES)), RpPickResult()
            winners = {}

            def pick_call(with_planes, tag):
                rc = pk._lib.rp_pick_select(pk._h, C.byref(p), C.byref(cost), 1, K, N_POSES, *[dptr(q) for q in planes], lens.ctypes.data_as(ip), None, 0,
                                            *[dptr(q) if with_planes else None for q in outs], status.ctypes.data_as(up), dptr(costs), None, None,
                                            C.byref(result), dptr(block))
                assert rc == 0, rc
                winners[tag] = int(result.best)

            l_outs = [np.empty((K, N_POSES)) for _ in range(8)]
            l_status, counts, ff, nf, first_free, n_hit = np.empty(K, np.uint32), np.zeros(8, np.int64), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()

            def chain_call():
                rc = lf._lib.rp_lift_evaluate(lf._h, C.byref(p), K, N_POSES, *[dptr(q) for q in planes], lens.ctypes.data_as(ip), None, 0,
                                              *[dptr(q) for q in l_outs], l_status.ctypes.data_as(up), C.byref(ff), C.byref(nf), counts.ctypes.data_as(lp))
                assert rc == 0, rc
                feasible = np.flatnonzero(l_status == 1)
                fl = lens[feasible]
                c = _default_cost(cost, fl, planes[0][feasible], planes[3][feasible], l_outs[3][feasible], l_outs[4][feasible], l_outs[7][feasible])
                order = feasible[np.argsort(c, kind="stable")]
                x, y, th, ol = (np.ascontiguousarray(q[order]) for q in (l_outs[0], l_outs[1], l_outs[2], lens))
                rc = ck._lib.rp_checker_check(ck._h, C.byref(p), 1, len(order), N_POSES, dptr(x), dptr(y), dptr(th), ol.ctypes.data_as(ip), None, None,
                                              None, C.byref(first_free), C.byref(n_hit))
                assert rc == 0, rc
                winners["c"] = int(order[first_free.value]) if first_free.value >= 0 else -1

            a_t, c_t = [], []
            for r in range(WARMUP + REPS):   # (a) and (c) alternate
                ta, tc = _clock(lambda: pick_call(False, "a")), _clock(chain_call)
                if r >= WARMUP:
                    a_t.append(ta)
                    c_t.append(tc)
            b_t = [_clock(lambda: pick_call(True, "b")) for _ in range(WARMUP + REPS)][WARMUP:]
            assert winners["a"] == winners["b"] == winners["c"] >= 0, winners
            res[str(K)] = {"a": _stats(a_t), "b": _stats(b_t), "c": _stats(c_t), "winner": winners["a"], "n_feasible": int(result.n_feasible),
                           "n_collision": int(result.n_collision), "before": int(result.n_collision_before_best)}
    print("RESULT " + json.dumps(res))


def _child(step):
    """One GPU step in a fresh process under its own time limit; None when it failed"""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"step {step}: time limit of {STEP_LIMIT_S} s", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"step {step}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", file=sys.stderr)
        return None
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        return {"pick": step_pick}[sys.argv[2]]()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "pick_batch.txt")
    got = _child("pick")
    if got is None:
        return 1
    src = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_pick.hip")
    digest = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
    fmt = lambda q: f"{q[0]:9.1f} us {q[1]:9.1f} us {q[2]:9.1f} us {q[3]:9.1f} us"   # noqa: E731
    first = got[str(KS[0])]
    lines = [f"rp_pick_select: K trajectories of {N_POSES} poses (own lengths) along the cfg2_ref_draw path ({len(np.load(FIXTURE)['ref_pos'])} vertices, rows in "
             f"LDS), the fixture's 64 stored trajectories repeated to K, its five dynamic obstacles, per-pose test",
             f"source: csrc/rp_pick.hip sha256 {digest}   date: {datetime.date.today().isoformat()}",
             f"wall time per call (host copies, kernels, copy back, synchronise) over {REPS} calls after {WARMUP} warm-up calls, one process, (a) and (c) "
             f"alternating; at K = 64: {first['n_feasible']} feasible, {first['n_collision']} of them colliding, {first['before']} in front of winner "
             f"{first['winner']}; (a), (b) and (c) name the same winner at every K",
             f"{'call':<62} {'median':>12} {'p10':>12} {'p90':>12} {'min':>12}"]
    for K in KS:
        g = got[str(K)]
        lines.append(f"{'(a) rp_pick_select, NULL planes K = ' + str(K):<62} {fmt(g['a'])}")
        lines.append(f"{'(b) rp_pick_select, all eight planes K = ' + str(K):<62} {fmt(g['b'])}")
        lines.append(f"{'(c) lift, NumPy cost, argsort, check in cost order K = ' + str(K):<62} {fmt(g['c'])}")
    for K in KS[1:]:
        g = got[str(K)]
        holds = g["a"][2] < g["c"][1]
        lines.append(f"THE CLAIM at K = {K}: (a) p90 {g['a'][2]:.1f} us {'<' if holds else '>='} (c) p10 {g['c'][1]:.1f} us: "
                     f"{'holds' if holds else 'DOES NOT HOLD'} (medians: (c) / (a) = {g['c'][0] / g['a'][0]:.2f})")
    lines.append(f"K = {KS[0]} is launch-bound on both sides and only reported.")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
