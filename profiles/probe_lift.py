"""Lift: time of one rp_lift_evaluate call on K = 64, 1 024 and 16 384 trajectories of 31 poses along the cfg2_ref_draw path (the 64
stored trajectories of tests/golden/cfg2_ref_draw.npz, rows s, d and their derivatives over each one's own length, repeated to K).
Beside it, on the same machine: (a) the host loop over CoordinateSystem.convert_to_cartesian_coords for the positions alone, and (b)
rp_plan_coeffs + rp_fetch_states for K polynomial candidates of the same size (the fixture's 64 coefficient pairs repeated to K) --
the one other way to get such rows from the device, open only to quartic / quintic pairs.
C calls on caller-owned arrays (and, for the lift, the binding's call that allocates its results), wall time around a call that ends in
the library's stream synchronise; warm-up calls first, then median, 10th and 90th percentile and minimum over the timed calls.
Every GPU step is a child process under its own time limit; the first step that fails ends the probe; nothing is tried twice.
usage (GPU box): python profiles/probe_lift.py [output file, default profiles/lift_batch.txt]"""
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
STEP_LIMIT_S = 240
FIXTURE = os.path.join(REPO, "tests", "golden", "cfg2_ref_draw.npz")


def _fixture():
    from commonroad_rp_amd._capi import FLAG_MATERIALIZE_ALL, make_cost, make_params
    z = dict(np.load(FIXTURE))
    veh = z["vehicle"]
    p = make_params(dt=float(z["dt"]), N=int(z["N"]), factor=int(z["factor"]), time_step0=int(z["time_step0"]), low_vel_mode=bool(z["low_vel_mode"]),
                    lon_mode=int(z["lon_mode"]), constraint_mask=int(z["constraint_mask"]), x0_lon=z["x0_lon"], x0_lat=z["x0_lat"],
                    x0_orientation=float(z["x0_orientation"]), wheelbase=veh[0], wb_rear_axle=veh[1], length=veh[2], width=veh[3], a_max=veh[4],
                    v_switch=veh[5], delta_max=veh[6], v_delta_max=veh[7], flags=FLAG_MATERIALIZE_ALL)
    ds, dss = float(z["desired_speed"]), float(z["desired_s"])
    cost = make_cost(kind=int(z["cost_kind"]), w_a=float(z["w_a"]), desired_speed=None if np.isnan(ds) else ds, desired_d=float(z["desired_d"]),
                     desired_s=None if np.isnan(dss) else dss)
    t_index = z["state_index"] // (len(z["L"]) * len(z["D"]))
    assert z["states"].shape[2] == N_POSES
    return z, p, cost, t_index


def _stats(samples):
    a = np.asarray(samples) * 1e6
    return [float(np.median(a)), float(np.percentile(a, 10)), float(np.percentile(a, 90)), float(a.min())]


def _timed(fn):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return _stats(out)


def step_lift():
    from commonroad_rp_amd import lift as lf_mod
    from commonroad_rp_amd._capi import dptr
    z, p, _, t_index = _fixture()
    lens64 = z["traj_len"][t_index].astype(np.int32)
    up, lp, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    res = {}
    with lf_mod.TrajectoryLifter(0) as lf:
        lf.set_reference(z["ref_path"], z["ref_pos"], z["ref_theta"], z["ref_curv"], z["ref_curv_d"], float(z["proj_d_limit"]))
        for K in KS:
            planes = [np.ascontiguousarray(np.tile(z["states"][:, r], (K // 64, 1))) for r in (7, 10, 11, 8, 12, 13)]
            lens = np.ascontiguousarray(np.tile(lens64, K // 64))
            outs = [np.empty((K, N_POSES)) for _ in range(8)]
            status, counts, ff, nf = np.empty(K, np.uint32), np.zeros(8, np.int64), C.c_int64(), C.c_int64()

            def c_call():
                rc = lf._lib.rp_lift_evaluate(lf._h, C.byref(p), K, N_POSES, *[dptr(q) for q in planes], lens.ctypes.data_as(ip), None, 0,
                                              *[dptr(q) for q in outs], status.ctypes.data_as(up), C.byref(ff), C.byref(nf), counts.ctypes.data_as(lp))
                assert rc == 0, rc

            def binding_call():
                lf.lift(p, *planes, lengths=lens)

            res[str(K)] = {"c": _timed(c_call), "binding": _timed(binding_call), "n_feasible": int(nf.value), "first_feasible": int(ff.value),
                           "counts": counts[1:7].tolist()}
    print("RESULT " + json.dumps(res))


def step_plan_coeffs():
    from commonroad_rp_amd._capi import RpContext
    z, p, cost, t_index = _fixture()
    res = {}
    ctx = RpContext(0)
    ctx.set_reference(z["ref_pos"], z["ref_theta"], z["ref_curv"], z["ref_curv_d"], z["ref_path"], float(z["proj_d_limit"]))
    ctx.set_obstacles(None)
    for K in KS:
        lon, lat = np.tile(z["lon_coeffs"], (K // 64, 1)), np.tile(z["lat_coeffs"], (K // 64, 1))
        T, tl = np.tile(z["T"][t_index], K // 64), np.tile(z["traj_len"][t_index], K // 64).astype(np.int32)

        def call():
            ctx.plan_coeffs(p, cost, lon, lat, T, tl, want_best_states=False)
            ctx.fetch_states(0, K)

        res[str(K)] = {"both": _timed(call)}
    ctx.close()
    print("RESULT " + json.dumps(res))


def host_loop():
    """(a): the scalar Python function, once per point, over the 64 stored trajectories; microseconds per point"""
    from commonroad_rp_amd.coordinate_system import CoordinateSystem
    z, _, _, t_index = _fixture()
    co = CoordinateSystem(z["ref_path"], proj_domain_d_limit=float(z["proj_d_limit"]))
    s, d, lens = z["states"][:, 7], z["states"][:, 8], z["traj_len"][t_index]
    pts = [(float(s[k, i]), float(d[k, i])) for k in range(64) for i in range(int(lens[k]))]
    for a, b in pts[:200]:
        co.convert_to_cartesian_coords(a, b)
    t0 = time.perf_counter()
    for a, b in pts:
        co.convert_to_cartesian_coords(a, b)
    return (time.perf_counter() - t0) / len(pts) * 1e6, len(pts), float(np.mean(lens))


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
        return {"lift": step_lift, "plan_coeffs": step_plan_coeffs}[sys.argv[2]]()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "lift_batch.txt")
    lift = _child("lift")
    if lift is None:
        return 1
    coeffs = _child("plan_coeffs")
    if coeffs is None:
        return 1
    us_point, n_pts, mean_len = host_loop()
    src = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_lift.hip")
    digest = hashlib.sha256(open(src, "rb").read()).hexdigest()[:16]
    fmt = lambda q: f"{q[0]:9.1f} us {q[1]:9.1f} us {q[2]:9.1f} us {q[3]:9.1f} us"   # noqa: E731
    lines = [f"rp_lift_evaluate: K trajectories of {N_POSES} poses (own lengths, {mean_len:.1f} on average) along the cfg2_ref_draw path "
             f"({len(np.load(FIXTURE)['ref_pos'])} vertices, rows in LDS), the fixture's 64 stored trajectories repeated to K",
             f"source: csrc/rp_lift.hip sha256 {digest}   date: {datetime.date.today().isoformat()}",
             f"wall time per call (host copies, kernels, copy back of all eight planes, synchronise) over {REPS} calls after {WARMUP} warm-up calls, "
             f"one process per library; feasible at K = 64: {lift['64']['n_feasible']}, reason counts {lift['64']['counts']}",
             f"{'call':<54} {'median':>12} {'p10':>12} {'p90':>12} {'min':>12}"]
    for K in KS:
        lines.append(f"{'rp_lift_evaluate K = ' + str(K):<54} {fmt(lift[str(K)]['c'])}")
    lines.append("THE CLAIM OF THIS CHANGE -- one lift call, median: " + ", ".join(f"K = {K}: {lift[str(K)]['c'][0]:.1f} us" for K in KS))
    lines.append("beside it (observations, not requirements: no threshold is set on any of these):")
    for K in KS:
        lines.append(f"{'TrajectoryLifter.lift (allocates its results) K = ' + str(K):<54} {fmt(lift[str(K)]['binding'])}")
    for K in KS:
        lines.append(f"{'(b) rp_plan_coeffs + rp_fetch_states K = ' + str(K):<54} {fmt(coeffs[str(K)]['both'])}")
    lines.append(f"(a) CoordinateSystem.convert_to_cartesian_coords in a Python loop, positions alone: {us_point:.2f} us per point over {n_pts} points = "
                 + ", ".join(f"{us_point * K * mean_len / 1e3:.1f} ms for K = {K}" for K in KS))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
