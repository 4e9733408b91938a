"""Ensemble collision check: one rp_ensemble_check call (both tests, every output) against the only way to ask the same question
without it, a loop of M x (TrajectoryChecker.set_obstacles + .check) on librp_check.so.  The scene generator and the timing method are
those of profiles/probe_check_batch.py: 61 poses, 50 dynamic obstacles, 99 static shapes, median wall time after warm-up.  K in
{64, 1024} trajectories, M in {8, 64} members; member m > 0 is the base table with every obstacle's track shifted by one N(0, 2 m)
draw.  Also: M = 1 beside rp_checker_check, and the values of EN_MEMBER_BLOCK (`make -C commonroad-reactive-planner_amd/csrc
ensemble-probe-variants` builds them into lib/ensemble_probe/; without them that table is left out).
usage (GPU box): python profiles/probe_ensemble.py [output file, default profiles/ensemble_batch.txt]"""
import ctypes as C
import datetime
import glob
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd"), os.path.join(REPO, "profiles")]
from commonroad_rp_amd import ensemble_check as ec   # noqa: E402
from commonroad_rp_amd import trajectory_check as tc   # noqa: E402
from commonroad_rp_amd._capi import dptr, make_params   # noqa: E402
from commonroad_rp_amd.collision import ObstacleTables   # noqa: E402
from probe_check_batch import N_DYN, N_POSES, N_STATIC, SCATTER, median_seconds, scene   # noqa: E402

KS, MS, SIGMA, REPS = (64, 1024), (8, 64), 2.0, 30
VARIANT_DIR = os.path.join(os.path.dirname(ec.LIB_PATH), "ensemble_probe")
SOURCE = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_ensemble.hip")
ip = C.POINTER(C.c_int32)


def make_members(rng, dyn, M):
    out = np.repeat(dyn[None], M, axis=0)
    for m in range(1, M):
        out[m, :, :, 0:2] += rng.normal(0.0, SIGMA, (dyn.shape[0], 1, 2))
    return out


class RawCall:
    """rp_ensemble_check as a C caller makes it, on caller-owned arrays; lean: the counts and the reduced answers only."""

    def __init__(self, en, p, x, y, th, M, lean=False):
        K = x.shape[0]
        self.en, self.p, self.x, self.y, self.th, self.K = en, p, x, y, th, K
        self.first_pose, self.first_seg = (None, None) if lean else (np.empty((K, M), np.int32), np.empty((K, M), np.int32))
        self.members_hit, self.ff, self.no = np.empty(K, np.int32), C.c_int64(), C.c_int64()

    def __call__(self):
        a = lambda v: v.ctypes.data_as(ip) if v is not None else None   # noqa: E731
        rc = self.en._lib.rp_ensemble_check(self.en._h, C.byref(self.p), ec.TRAJ_POSES | ec.TRAJ_SWEPT, self.K, N_POSES, dptr(self.x), dptr(self.y),
                                            dptr(self.th), None, 0, a(self.first_pose), a(self.first_seg), a(self.members_hit), C.byref(self.ff),
                                            C.byref(self.no))
        assert rc == 0, rc


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "ensemble_batch.txt")
    p = make_params(dt=0.1, N=N_POSES - 1, factor=1, time_step0=2, x0_lon=[0, 0, 0], x0_lat=[0, 0, 0], x0_orientation=0.0, wheelbase=2.5789,
                    wb_rear_axle=1.4227, length=4.508, width=1.61, a_max=11.5, v_switch=7.319, delta_max=1.066, v_delta_max=0.4)
    kept = int(re.search(r"\bEN_MEMBER_BLOCK\s*=\s*(\d+)\s*;", open(SOURCE).read()).group(1))
    en, ck = ec.EnsembleChecker(0), tc.TrajectoryChecker(0)
    lines = [f"rp_ensemble_check (RP_TRAJ_POSES | RP_TRAJ_SWEPT, every output) against a loop of M x (TrajectoryChecker.set_obstacles + .check); "
             f"{N_POSES} poses, {N_DYN} dynamic obstacles, {N_STATIC} static shapes scattered {SCATTER:.0f} m around the poses; member m > 0: every "
             f"track shifted by one N(0, {SIGMA:.0f} m) draw",
             f"library: {os.path.relpath(ec.LIB_PATH, REPO)} (EN_MEMBER_BLOCK = {kept}); the loop: {os.path.relpath(tc.LIB_PATH, REPO)}   "
             f"date: {datetime.date.today().isoformat()}",
             f"median wall time per call over {REPS} calls after 3 warm-up calls; lean: members_hit, first_free and n_over only (no [K][M] matrix comes back)",
             f"{'K':>6} {'M':>4} {'over 0':>7} {'ensemble C call':>16} {'.check()':>12} {'lean C call':>12} {'loop of M':>13} {'loop / C call':>14}"]
    scenes = {}
    for K in KS:
        x, y, th, obs = scene(np.random.default_rng(K), K)
        for M in MS:
            members = make_members(np.random.default_rng(1000 * K + M), obs.dyn_obb, M)
            scenes[K, M] = (x, y, th, obs, members)
            en.set_obstacles(obs, members, obs.dyn_t0)
            raw, lean = RawCall(en, p, x, y, th, M), RawCall(en, p, x, y, th, M, lean=True)
            member_tables = [ObstacleTables(static_obb=obs.static_obb, static_tri=obs.static_tri, static_circ=obs.static_circ, dyn_obb=members[m],
                                            dyn_t0=obs.dyn_t0) for m in range(M)]

            def loop():
                out = []
                for tb in member_tables:
                    ck.set_obstacles(tb)
                    out.append(ck.check(p, x, y, th, poses=True, swept=True))
                return out
            t_raw, t_lean = median_seconds(raw, REPS), median_seconds(lean, REPS)
            t_py = median_seconds(lambda: en.check(p, x, y, th, poses=True, swept=True), REPS)
            t_loop = median_seconds(loop, 10 if M > 8 else REPS)
            ref = loop()
            assert all(np.array_equal(raw.first_pose[:, m], r.first_pose_hit) and np.array_equal(raw.first_seg[:, m], r.first_segment_hit)
                       for m, r in enumerate(ref)), "the ensemble call and the loop of checker calls disagree"
            assert np.array_equal(raw.members_hit, lean.members_hit) and (raw.ff.value, raw.no.value) == (lean.ff.value, lean.no.value)
            lines.append(f"{K:6d} {M:4d} {raw.no.value:7d} {t_raw * 1e6:13.1f} us {t_py * 1e6:9.1f} us {t_lean * 1e6:9.1f} us {t_loop * 1e6:10.1f} us "
                         f"{t_loop / t_raw:14.1f}")
            print(lines[-1], flush=True)
    lines += ["", "M = 1 (set_obstacles(tables)) beside rp_checker_check on the same scene, C calls, first-hit arrays and reduced answers",
              f"{'K':>6} {'rp_ensemble_check':>18} {'rp_checker_check':>17} {'ratio':>7}"]
    for K in KS:
        x, y, th, obs, _ = scenes[K, MS[0]]
        en.set_obstacles(obs)
        ck.set_obstacles(obs)
        raw = RawCall(en, p, x, y, th, 1)
        first_pose, first_seg, ff, nh = np.empty(K, np.int32), np.empty(K, np.int32), C.c_int64(), C.c_int64()

        def checker():
            rc = ck._lib.rp_checker_check(ck._h, C.byref(p), tc.TRAJ_POSES | tc.TRAJ_SWEPT, K, N_POSES, dptr(x), dptr(y), dptr(th), None,
                                          first_pose.ctypes.data_as(ip), first_seg.ctypes.data_as(ip), None, C.byref(ff), C.byref(nh))
            assert rc == 0, rc
        t_en, t_ck = median_seconds(raw, REPS), median_seconds(checker, REPS)
        assert np.array_equal(raw.first_pose[:, 0], first_pose) and np.array_equal(raw.first_seg[:, 0], first_seg) and raw.no.value == nh.value
        lines.append(f"{K:6d} {t_en * 1e6:15.1f} us {t_ck * 1e6:14.1f} us {t_en / t_ck:7.2f}")
        print(lines[-1], flush=True)
    en.close()
    ck.close()
    variants = sorted(glob.glob(os.path.join(VARIANT_DIR, "librp_ensemble_b*.so")), key=lambda f: int(re.search(r"_b(\d+)\.so$", f).group(1)))
    if variants:
        combos = [(K, M) for K in KS for M in MS]
        lines += ["", f"EN_MEMBER_BLOCK: the ensemble C call (every output) on libraries built with -DEN_MEMBER_BLOCK_PROBE=<n>, two passes over "
                      f"the values, median of {REPS} calls each; kept: {kept}",
                  f"{'block':>6} {'pass':>5} " + " ".join(f"{f'K={K} M={M}':>14}" for K, M in combos)]
        for rep in range(2):
            for path in variants:
                block = int(re.search(r"_b(\d+)\.so$", path).group(1))
                with ec.EnsembleChecker(0, library=path) as var:
                    t = []
                    for K, M in combos:
                        x, y, th, obs, members = scenes[K, M]
                        var.set_obstacles(obs, members, obs.dyn_t0)
                        t.append(median_seconds(RawCall(var, p, x, y, th, M), REPS))
                lines.append(f"{block:6d} {rep:5d} " + " ".join(f"{v * 1e6:11.1f} us" for v in t))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:4]))


if __name__ == "__main__":
    main()
