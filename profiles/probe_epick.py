"""Pick under a risk bound: time of one rp_epick_select call on K = 64, 1 024 and 16 384 trajectories of 31 poses along the cfg2_ref_draw
path (the 64 stored trajectories of tests/golden/cfg2_ref_draw.npz repeated to K, as in profiles/pick_batch.txt) against M = 1, 8 and 64
members -- member 0 is that fixture's table of five dynamic obstacles, in member m > 0 every obstacle's track is shifted by one N(0, 2 m)
draw in x and y --, per-pose test, dyadic member weights (1, 2 or 3 sixty-fourths: their sums are exact in any order), max_risk a quarter
of the total weight --
  (a) rp_epick_select with NULL planes and NULL first-hit matrices: status, cost, members_hit, risk, the scalars and the winner's block
      come back;
  (c) the chain it replaces, in the same process and alternating with (a) call by call, every step an existing call: rp_pick_select
      with mode 0 returning x, y and theta, rp_ensemble_check on the feasible rows returning the [K][M] first-hit matrix, and the
      weights product, the mask and the argmin in NumPy;
  (p) at M = 1, rp_pick_select on the same inputs and member 0 as its table: (a) - (p) is the price of the member dimension.
(a) and (c) must name the same winner; the run fails otherwise.  With libraries built by `make epick-probe-variants`, (a) is also timed
at M = 8 for each value of EP_MEMBER_BLOCK.
C calls on caller-owned arrays, wall time around a call that ends in the library's stream synchronise; warm-up calls first, then median,
10th and 90th percentile and minimum over the timed calls.  THE CLAIM: (a) is faster than (c) at K = 1 024 and K = 16 384 for M = 8,
which holds at a size when (a)'s p90 is below (c)'s p10; K = 64 is launch-bound on both sides and only reported.
The GPU step is a child process under its own time limit; nothing is tried twice.  Fails without a GPU.
usage (GPU box): python profiles/probe_epick.py [output file, default profiles/epick_batch.txt]"""
import ctypes as C
import datetime
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd")]

from probe_pick import FIXTURE, N_POSES, _clock, _fixture, _stats   # noqa: E402  (the same inputs as profiles/pick_batch.txt)

KS, MS, REPS, WARMUP = (64, 1024, 16384), (1, 8, 64), 100, 10
CLAIM_M = 8
STEP_LIMIT_S = 500
SOURCE = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_epick.hip")
VARIANTS = os.path.join(REPO, "commonroad-reactive-planner_amd", "lib", "epick_probe")
MEMBER_SIGMA = 2.0


def _members(dyn, M):
    rng = np.random.default_rng([7, M])
    out = np.repeat(dyn[None], M, axis=0)
    for m in range(1, M):
        out[m, :, :, 0:2] += rng.normal(0.0, MEMBER_SIGMA, (dyn.shape[0], 1, 2))
    return np.ascontiguousarray(out)


def _weights(M):
    return (1.0 + np.arange(M) % 3) / 64.0


def _variant_libraries():
    if not os.path.isdir(VARIANTS):
        return {}
    found = {}
    for name in sorted(os.listdir(VARIANTS)):
        m = re.fullmatch(r"librp_epick_b(\d+)\.so", name)
        if m:
            found[int(m.group(1))] = os.path.join(VARIANTS, name)
    return found


def step_epick():
    from commonroad_rp_amd import EnsembleChecker, EnsemblePicker, TrajectoryPicker
    from commonroad_rp_amd._capi import dptr
    from commonroad_rp_amd.ensemble_pick import RpEpickResult
    from commonroad_rp_amd.pick import RpPickResult
    z, p, cost, obs, t_index = _fixture()
    lens64 = z["traj_len"][t_index].astype(np.int32)
    up, lp, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    tables = (z["ref_path"], z["ref_pos"], z["ref_theta"], z["ref_curv"], z["ref_curv_d"], float(z["proj_d_limit"]))
    res = {}

    def epick_call(ep, K, planes, lens, bound, out):
        status, costs, hit, risk, block, result = out
        rc = ep._lib.rp_epick_select(ep._h, C.byref(p), C.byref(cost), 1, bound, K, N_POSES, *[dptr(q) for q in planes], lens.ctypes.data_as(ip), None, 0,
                                     *([None] * 8), status.ctypes.data_as(up), dptr(costs), hit.ctypes.data_as(ip), dptr(risk), None, None,
                                     C.byref(result), dptr(block))
        assert rc == 0, rc
        return int(result.best)

    with EnsemblePicker(0) as ep, TrajectoryPicker(0) as pk, EnsembleChecker(0) as en:
        for q in (ep, pk):
            q.set_reference(*tables)
        ep.set_static(obs)
        en.set_static(obs)
        pk.set_obstacles(obs)
        for M in MS:
            members, w = _members(obs.dyn_obb, M), _weights(M)
            bound = 0.25 * float(w.sum())
            ep.set_members(members, obs.dyn_t0, w)
            en.set_members(members, obs.dyn_t0)
            for K in KS:
                planes = [np.ascontiguousarray(np.tile(z["states"][:, r], (K // 64, 1))) for r in (7, 10, 11, 8, 12, 13)]
                lens = np.ascontiguousarray(np.tile(lens64, K // 64))
                out = (np.empty(K, np.uint32), np.empty(K), np.empty(K, np.int32), np.empty(K), np.empty((14, N_POSES)), RpEpickResult())
                x, y, th = (np.empty((K, N_POSES)) for _ in range(3))
                c_status, c_costs, c_result = np.empty(K, np.uint32), np.empty(K), RpPickResult()
                winners = {}

                def a_call():
                    winners["a"] = epick_call(ep, K, planes, lens, bound, out)

                def chain_call():
                    rc = pk._lib.rp_pick_select(pk._h, C.byref(p), C.byref(cost), 0, K, N_POSES, *[dptr(q) for q in planes], lens.ctypes.data_as(ip), None,
                                                0, dptr(x), dptr(y), dptr(th), *([None] * 5), c_status.ctypes.data_as(up), dptr(c_costs), None, None,
                                                None, None)
                    assert rc == 0, rc
                    feasible = np.flatnonzero(c_status == 1)
                    fx, fy, fth, fl = (np.ascontiguousarray(q[feasible]) for q in (x, y, th, lens))
                    first = np.empty((len(feasible), M), np.int32)
                    rc = en._lib.rp_ensemble_check(en._h, C.byref(p), 1, len(feasible), N_POSES, dptr(fx), dptr(fy), dptr(fth), fl.ctypes.data_as(ip), M,
                                                   first.ctypes.data_as(ip), None, None, None, None)
                    assert rc == 0, rc
                    risk = (first >= 0) @ w
                    masked = np.where(risk <= bound, c_costs[feasible], np.inf)
                    best = int(np.argmin(masked)) if len(feasible) else -1
                    winners["c"] = int(feasible[best]) if best >= 0 and np.isfinite(masked[best]) else -1

                def pick_call():
                    rc = pk._lib.rp_pick_select(pk._h, C.byref(p), C.byref(cost), 1, K, N_POSES, *[dptr(q) for q in planes], lens.ctypes.data_as(ip), None,
                                                0, *([None] * 8), c_status.ctypes.data_as(up), dptr(c_costs), None, None, C.byref(c_result), dptr(out[4]))
                    assert rc == 0, rc

                a_t, c_t = [], []
                for r in range(WARMUP + REPS):   # (a) and (c) alternate
                    ta, tc = _clock(a_call), _clock(chain_call)
                    if r >= WARMUP:
                        a_t.append(ta)
                        c_t.append(tc)
                assert winners["a"] == winners["c"], (M, K, winners)
                result = out[5]
                g = {"a": _stats(a_t), "c": _stats(c_t), "winner": winners["a"], "n_feasible": int(result.n_feasible), "n_collision": int(result.n_collision),
                     "before": int(result.n_collision_before_best), "best_hit": int(result.best_members_hit)}
                if M == 1:
                    a_t, p_t = [], []
                    for r in range(WARMUP + REPS):   # (a) and (p) alternate
                        ta, tp = _clock(a_call), _clock(pick_call)
                        if r >= WARMUP:
                            a_t.append(ta)
                            p_t.append(tp)
                    g["a1"], g["p"] = _stats(a_t), _stats(p_t)
                res[f"{M},{K}"] = g
    # the member block: (a) at M = CLAIM_M on libraries built with other values of EP_MEMBER_BLOCK, alternating among them
    blocks = _variant_libraries()
    if blocks:
        members, w = _members(obs.dyn_obb, CLAIM_M), _weights(CLAIM_M)
        bound = 0.25 * float(w.sum())
        pickers = {}
        for b, path in blocks.items():
            pickers[b] = EnsemblePicker(0, library=path)
            pickers[b].set_reference(*tables)
            pickers[b].set_static(obs)
            pickers[b].set_members(members, obs.dyn_t0, w)
        for K in KS[1:]:
            planes = [np.ascontiguousarray(np.tile(z["states"][:, r], (K // 64, 1))) for r in (7, 10, 11, 8, 12, 13)]
            lens = np.ascontiguousarray(np.tile(lens64, K // 64))
            out = (np.empty(K, np.uint32), np.empty(K), np.empty(K, np.int32), np.empty(K), np.empty((14, N_POSES)), RpEpickResult())
            times = {b: [] for b in blocks}
            for r in range(WARMUP + REPS):
                for b in blocks:
                    t = _clock(lambda: epick_call(pickers[b], K, planes, lens, bound, out))
                    if r >= WARMUP:
                        times[b].append(t)
            for b in blocks:
                res[f"block{b},{K}"] = _stats(times[b])
        for q in pickers.values():
            q.close()
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
        return {"epick": step_epick}[sys.argv[2]]()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "epick_batch.txt")
    got = _child("epick")
    if got is None:
        return 1
    text = open(SOURCE).read()
    digest = hashlib.sha256(text.encode()).hexdigest()[:16]
    block = int(re.search(r"#else\s*\n\s*constexpr int EP_MEMBER_BLOCK\s*=\s*(\d+);", text).group(1))
    fmt = lambda q: f"{q[0]:9.1f} us {q[1]:9.1f} us {q[2]:9.1f} us {q[3]:9.1f} us"   # noqa: E731
    lines = [f"rp_epick_select: K trajectories of {N_POSES} poses (own lengths) along the cfg2_ref_draw path ({len(np.load(FIXTURE)['ref_pos'])} vertices, rows "
             f"in LDS), the fixture's 64 stored trajectories repeated to K, M members of its five dynamic obstacles (member 0 the fixture's table, the others "
             f"shifted by N(0, {MEMBER_SIGMA:g} m) per obstacle), per-pose test, weights 1 .. 3 sixty-fourths, max_risk a quarter of their sum",
             f"source: csrc/rp_epick.hip sha256 {digest}, EP_MEMBER_BLOCK = {block}   date: {datetime.date.today().isoformat()}",
             f"wall time per call (host copies, kernels, copy back, synchronise) over {REPS} calls after {WARMUP} warm-up calls, one process, (a) and (c) "
             f"alternating; (a) and (c) name the same winner at every size",
             f"{'call':<78} {'median':>12} {'p10':>12} {'p90':>12} {'min':>12}"]
    for M in MS:
        for K in KS:
            g = got[f"{M},{K}"]
            lines.append(f"M = {M}, K = {K}: {g['n_feasible']} feasible, {g['n_collision']} of them over the bound, {g['before']} in front of winner {g['winner']} "
                         f"(which collides in {g['best_hit']} members)")
            lines.append(f"{'(a) rp_epick_select, NULL planes and matrices M = ' + str(M) + ', K = ' + str(K):<78} {fmt(g['a'])}")
            lines.append(f"{'(c) pick without test, ensemble check, NumPy weights and argmin M = ' + str(M) + ', K = ' + str(K):<78} {fmt(g['c'])}")
    for K in KS[1:]:
        g = got[f"{CLAIM_M},{K}"]
        holds = g["a"][2] < g["c"][1]
        lines.append(f"THE CLAIM at M = {CLAIM_M}, K = {K}: (a) p90 {g['a'][2]:.1f} us {'<' if holds else '>='} (c) p10 {g['c'][1]:.1f} us: "
                     f"{'holds' if holds else 'DOES NOT HOLD'} (medians: (c) / (a) = {g['c'][0] / g['a'][0]:.2f})")
    lines.append(f"K = {KS[0]} is launch-bound on both sides and only reported.")
    lines.append("The price of the member dimension, M = 1: (a) beside (p) rp_pick_select with the per-pose test on the same inputs and member 0 as its table, "
                 "alternating")
    for K in KS:
        g = got[f"1,{K}"]
        lines.append(f"{'(a) rp_epick_select, NULL planes and matrices M = 1, K = ' + str(K):<78} {fmt(g['a1'])}")
        lines.append(f"{'(p) rp_pick_select, NULL planes K = ' + str(K):<78} {fmt(g['p'])}")
        lines.append(f"  medians: (a) - (p) = {g['a1'][0] - g['p'][0]:.1f} us")
    blocks = sorted(int(k.split(",")[0][5:]) for k in got if k.startswith("block") and k.endswith(f",{KS[1]}"))
    if blocks:
        lines.append(f"The member block: (a) at M = {CLAIM_M} on libraries built with -DEP_MEMBER_BLOCK_PROBE=<b> (make epick-probe-variants), alternating "
                     f"among them; a wavefront walks the members of its block one after the other (ck_pose_hit unchanged per member)")
        for K in KS[1:]:
            for b in blocks:
                lines.append(f"{'(a) EP_MEMBER_BLOCK = ' + str(b) + ', M = ' + str(CLAIM_M) + ', K = ' + str(K):<78} {fmt(got[f'block{b},{K}'])}")
    else:
        lines.append("The member block: no variant libraries (make epick-probe-variants) were present; only the built value was timed.")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
