"""Batch collision check of given trajectories: one rp_checker_check call (both tests) against the only way to ask the same question
without it, a loop of RpContext.check_swept (one trajectory, one workgroup, one device round trip per call).  K in {64, 1024, 16384}
trajectories of 61 poses, 50 dynamic obstacles, 99 static shapes.  The loop is timed over 64 trajectories and scaled linearly to K.
usage (GPU box): python profiles/probe_check_batch.py [output file, default profiles/check_batch.txt]"""
import ctypes as C
import datetime
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd")]
from commonroad_rp_amd import trajectory_check as tc   # noqa: E402
from commonroad_rp_amd._capi import RpContext, dptr, make_params   # noqa: E402
from commonroad_rp_amd.collision import ObstacleTables   # noqa: E402

N_POSES, N_DYN, N_STATIC, LOOP = 61, 50, 99, 64
SCATTER = 150.0   # metres: spread of the obstacles around the poses (between a third and two thirds of the trajectories collide)


def scene(rng, K):
    th = rng.uniform(-math.pi, math.pi) + rng.uniform(-0.5, 0.5, (K, 1)) + np.cumsum(rng.normal(0, 0.05, (K, N_POSES)), axis=1)
    v = rng.uniform(0.0, 30.0, (K, 1))
    x = rng.normal(0, 3.0, (K, 1)) + np.cumsum(v * 0.1 * np.cos(th), axis=1)
    y = rng.normal(0, 3.0, (K, 1)) + np.cumsum(v * 0.1 * np.sin(th), axis=1)
    dyn = np.full((N_DYN, N_POSES + 8, 5), np.nan)
    for j in range(N_DYN):
        k, off = rng.integers(0, K), rng.normal(0, SCATTER, 2)
        for q in range(dyn.shape[1]):
            i = min(q, N_POSES - 1)
            dyn[j, q] = (x[k, i] + off[0] + 0.3 * q, y[k, i] + off[1], rng.uniform(-3, 3), rng.uniform(0.2, 2.5), rng.uniform(0.2, 1.2))
    sobb, tri, circ = [], [], []
    for j in range(N_STATIC):
        k, i = rng.integers(0, K), rng.integers(0, N_POSES)
        px, py = x[k, i] + rng.normal(0, SCATTER), y[k, i] + rng.normal(0, SCATTER)
        if j % 3 == 0:
            sobb.append([px, py, rng.uniform(-3, 3), rng.uniform(0.2, 6.0), rng.uniform(0.05, 1.0)])
        elif j % 3 == 1:
            tri.append([px, py, px + rng.uniform(0.2, 2), py + rng.uniform(-1, 1), px + rng.uniform(-1, 1), py + rng.uniform(0.2, 2)])
        else:
            circ.append([px, py, rng.uniform(0.1, 1.5)])
    return x, y, th, ObstacleTables(static_obb=sobb, static_tri=tri, static_circ=circ, dyn_obb=dyn, dyn_t0=0)


def median_seconds(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "check_batch.txt")
    p = make_params(dt=0.1, N=N_POSES - 1, factor=1, time_step0=2, x0_lon=[0, 0, 0], x0_lat=[0, 0, 0], x0_orientation=0.0, wheelbase=2.5789,
                    wb_rear_axle=1.4227, length=4.508, width=1.61, a_max=11.5, v_switch=7.319, delta_max=1.066, v_delta_max=0.4)
    ck, ctx = tc.TrajectoryChecker(0), RpContext(0)
    s = np.arange(0.0, 50.0, 1.0)
    ctx.set_reference(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0)
    lines = [f"rp_checker_check (RP_TRAJ_POSES | RP_TRAJ_SWEPT) against a loop of RpContext.check_swept; {N_POSES} poses, {N_DYN} dynamic obstacles, "
             f"{N_STATIC} static shapes scattered {SCATTER:.0f} m around the poses", f"library: {os.path.relpath(tc.LIB_PATH, REPO)}   date: {datetime.date.today().isoformat()}",
             "median wall time per call; the loop is timed over 64 trajectories and scaled linearly to K",
             f"{'K':>6} {'colliding':>9} {'batch C call':>13} {'batch .check()':>15} {'loop of 64':>11} {'loop scaled to K':>17} {'per trajectory: batch | loop':>30} {'ratio':>7}"]
    for K in (64, 1024, 16384):
        x, y, th, obs = scene(np.random.default_rng(K), K)
        ck.set_obstacles(obs)
        ctx.set_obstacles(obs)
        first_pose, first_seg = np.empty(K, np.int32), np.empty(K, np.int32)
        ff, nh = C.c_int64(), C.c_int64()
        ip = C.POINTER(C.c_int32)

        def raw():
            rc = ck._lib.rp_checker_check(ck._h, C.byref(p), tc.TRAJ_POSES | tc.TRAJ_SWEPT, K, N_POSES, dptr(x), dptr(y), dptr(th), None,
                                          first_pose.ctypes.data_as(ip), first_seg.ctypes.data_as(ip), None, C.byref(ff), C.byref(nh))
            assert rc == 0, rc

        def loop():
            return [ctx.check_swept(p, x[k], y[k], th[k]) for k in range(LOOP)]
        t_raw = median_seconds(raw, 30 if K < 16384 else 10)
        t_py = median_seconds(lambda: ck.check(p, x, y, th, poses=True, swept=True), 30 if K < 16384 else 10)
        t_loop = median_seconds(loop, 10)
        assert list(first_seg[:LOOP]) == loop(), "the batch call and rp_check_swept disagree"
        scaled = t_loop * K / LOOP
        lines.append(f"{K:6d} {nh.value:9d} {t_raw * 1e6:10.1f} us {t_py * 1e6:12.1f} us {t_loop * 1e6:8.1f} us {scaled * 1e6:14.1f} us "
                     f"{t_raw / K * 1e6:14.3f} | {t_loop / LOOP * 1e6:8.3f} us {scaled / t_raw:7.1f}")
        print(lines[-1], flush=True)
    ck.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4]))


if __name__ == "__main__":
    main()
