"""Shared by tests/test_pick_abi.py (CPU) and tests/test_pick.py (GPU): the yardstick of the pick (include/rp_pick.h).  Nothing here
is new arithmetic; it composes the references the project already trusts --

  ``_lift.reference``                                the eight planes and the kinematic status word,
  ``_score.cost_of``                                 the cost, on the reference's own v, a, theta_cl and the given s, d,
  ``oracle.check_poses`` / ``oracle.check_swept``    the first colliding pose / segment, on the reference's own x, y, theta,

-- and does the selection and the counts in plain Python.  Besides: the cases (inputs, obstacles, the reference's answer, computed
once per session and never written to) and the two conditions every case that runs on the GPU must meet (``knife_edges``)."""
import functools
import math
import os
import re
from types import SimpleNamespace as NS

import numpy as np

from commonroad_rp_amd._capi import RpParams
from commonroad_rp_amd.collision import ObstacleTables

import _lift as L
import _score as S

REPO = S.REPO
HEADER = os.path.join(REPO, "include", "rp_pick.h")
CSRC = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc")
SOURCE = os.path.join(CSRC, "rp_pick.hip")


def _constant(path, name, default):
    m = re.search(name + r"\s*=\s*(\d+)", open(path).read()) if os.path.exists(path) else None
    return int(m.group(1)) if m else default


LF_LDS_ROWS = _constant(SOURCE, "PK_LF_LDS_ROWS", 384)   # segment rows the lift kernel stages in LDS
CK_LDS_ROWS = _constant(SOURCE, "PK_CK_LDS_ROWS", 128)   # static shapes the collision kernel stages in LDS
POSES, SWEPT = 1, 2
EDGE = 2e-6        # both vehicle extents grown and shrunk by this much must leave every first hit where it is
COST_GAP = 1e-9    # smallest relative distance of a feasible trajectory's cost to the winner's (or exactly 0: a duplicate)
INPUT_ROWS = (L.RP_S, L.RP_S_DOT, L.RP_S_DDOT, L.RP_D, L.RP_D_DOT, L.RP_D_DDOT)   # rows of a state block the six input planes are
PLANE_ROWS = (0, 1, 2, 3, 4, 5, 6, L.RP_THETA_CL)                                 # ... and the eight lifted planes
DT = L.DT


# ---- the reference -------------------------------------------------------------------------------------------------------------
def oracle_tables(t, obs):
    from oracle.oracle import OracleTables
    return OracleTables(t.pos, t.theta, t.curv, t.curv_d, t.ref, t.d_limit, obs)


def first_hits(p, t, obs, o, mode, grow=0.0, theta=None):
    """(first_pose_hit, first_segment_hit), [K] int32 each, of the oracle on the reference's own poses: -1 where nothing hit, for a
    test that was not asked for and for a trajectory that is not kinematically feasible.  ``grow``: added to the vehicle's length and
    width; ``theta``: orientations in place of the reference's."""
    from oracle import oracle
    q = RpParams.from_buffer_copy(p)
    q.length, q.width = p.length + grow, p.width + grow
    tb = oracle_tables(t, obs)
    th = o.theta if theta is None else theta
    K = len(o.status)
    fp, fs = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    for k in np.flatnonzero(o.status == 1):
        n = int(o.lengths[k])
        if mode & POSES:
            h, _ = oracle.check_poses(q, tb, o.x[k, :n], o.y[k, :n], th[k, :n])
            fp[k] = np.flatnonzero(h)[0] if h.any() else -1
        if mode & SWEPT:
            fs[k] = oracle.check_swept(q, tb, o.x[k, :n], o.y[k, :n], th[k, :n])[0]
    return fp, fs


def select(status, cost):
    """(best, n_collision_before_best): the lexicographic minimum of (cost, k) over label 1 (a NaN cost never wins), and the
    trajectories with label 3 in front of it in that order -- all of them without a winner"""
    best = -1
    for k in np.flatnonzero((status & 3) == 1):
        if cost[k] == cost[k] and (best < 0 or cost[k] < cost[best]):
            best = int(k)
    hit = np.flatnonzero((status & 3) == 3)
    if best < 0:
        return best, int(hit.size)
    return best, int(sum(1 for k in hit if cost[k] < cost[best] or (cost[k] == cost[best] and k < best)))


def reference(p, cost, t, obs, planes, lengths=None, theta0=None, mode=POSES):
    """What rp_pick_select returns, as a namespace: lift (the namespace of ``_lift.reference``: planes, lengths), status, cost [K],
    first_pose_hit, first_segment_hit [K], best, best_cost, best_states ([14, n] or None), n_feasible, n_collision,
    n_collision_before_best, reason_counts [8]"""
    planes = [np.atleast_2d(np.asarray(q, float)) for q in planes]
    o = L.reference(p, t, *planes, lengths=lengths, theta0=theta0)
    K, n = planes[0].shape
    costs = np.full(K, np.nan)
    for k in np.flatnonzero(o.status == 1):
        m = int(o.lengths[k])
        costs[k] = S.cost_of(cost, o.a[k, :m], o.v[k, :m], planes[0][k, :m], planes[3][k, :m], o.theta_cl[k, :m])
    fp, fs = first_hits(p, t, obs, o, mode)
    status = o.status.copy()
    for k in np.flatnonzero((fp >= 0) | (fs >= 0)):
        status[k] = S.status_word(3, 0, min(int(fp[k] if fp[k] >= 0 else fs[k]), 0xFFF))
    best, before = select(status, costs)
    block = None
    if best >= 0:
        block = np.full((14, n), np.nan)
        m = int(o.lengths[best])
        for row, name in zip(PLANE_ROWS, L.PLANES):
            block[row] = getattr(o, name)[best]
        for row, q in zip(INPUT_ROWS, planes):
            block[row, :m] = q[best, :m]
    return NS(lift=o, status=status, cost=costs, first_pose_hit=fp, first_segment_hit=fs, best=best, best_cost=costs[best] if best >= 0 else math.nan,
              best_states=block, n_feasible=int((o.status == 1).sum()), n_collision=int(((status & 3) == 3).sum()), n_collision_before_best=before,
              reason_counts=o.reason_counts)


def knife_edges(c):
    """The two conditions of a case: (first hits unchanged with the vehicle EDGE longer and wider and EDGE shorter and narrower,
    smallest relative cost gap between the winner and another kinematically feasible trajectory that is not its bit-identical copy --
    inf without a winner or a rival)"""
    r = c.ref
    steady = True
    for grow in (EDGE, -EDGE):
        fp, fs = first_hits(c.p, c.path, c.obs, r.lift, c.mode, grow=grow)
        steady = steady and np.array_equal(fp, r.first_pose_hit) and np.array_equal(fs, r.first_segment_hit)
    gap = math.inf
    if r.best >= 0:
        m = int(r.lift.lengths[r.best])
        for k in np.flatnonzero(r.lift.status == 1):
            if k == r.best:
                continue
            same = r.lift.lengths[k] == m and all(np.array_equal(q[k, :m], q[r.best, :m]) for q in c.planes) and \
                (c.theta0 is None or c.theta0[k] == c.theta0[r.best])
            if same and r.cost[k] == r.best_cost:
                continue
            gap = min(gap, abs(r.cost[k] - r.best_cost) / abs(r.best_cost))
    return steady, gap


# ---- the pin: the reference planner's own decision -------------------------------------------------------------------------------
def fixture_obstacles(name):
    z = np.load(os.path.join(S.GOLDEN, name + ".npz"))
    return ObstacleTables(static_obb=z["static_obb"], static_tri=z["static_tri"], static_circ=z["static_circ"], dyn_obb=z["dyn_obb"], dyn_t0=int(z["dyn_t0"]))


def fixture_extras(name):
    z = np.load(os.path.join(S.GOLDEN, name + ".npz"))
    idx = z["state_index"]
    return NS(collide_all=z["collide_all"][idx].astype(int), winner=int(z["winner"]), winner_cost=float(z["winner_cost"]),
              n_infeasible_collision=int(z["n_infeasible_collision"]), n_infeasible_kinematics=int(z["n_infeasible_kinematics"]), index=idx)


@functools.lru_cache(maxsize=None)
def pin(name="arc_hv_l1_draw"):
    """A draw fixture fed whole: every stored block, rows RP_S .. RP_D_DDOT as the six planes over all N + 1 poses (the stored rows
    carry the planner's horizon extension), the fixture's obstacles, params and cost, the per-pose test"""
    f = S.fixture(name)
    planes = tuple(np.ascontiguousarray(f.states[:, row]) for row in INPUT_ROWS)
    for q in planes:
        q.setflags(write=False)
    c = NS(name="pin_" + name, p=f.p, cost=f.cost, path=L.fixture_path(name), obs=fixture_obstacles(name), planes=planes, lengths=None, theta0=None,
           mode=POSES, fixture=f, extras=fixture_extras(name))
    c.ref = reference(c.p, c.cost, c.path, c.obs, planes, mode=c.mode)
    return c


# ---- synthetic cases -------------------------------------------------------------------------------------------------------------
# name -> (K, n_poses); what each exercises is listed in tests/test_pick.py
CASES = {"n63": (2, 63), "n64": (2, 64), "n65": (2, 65), "n129": (2, 129), "ragged": (37, 65), "many": (1100, 21), "factor3": (8, 30),
         "standstill": (4, 80), "low_vel": (8, 40), "long_path": (16, 31), "many_static": (6, 30), "all_infeasible": (5, 20), "all_collide": (6, 25),
         "no_obstacles": (9, 21), "mode0": (6, 25), "duplicates": (8, 21)}
SEED = 2027
LINE_D = -1.25     # the lateral offset of a line of circles that nothing driving within 0.75 m of it passes


def _cruise(n, s0, v0, d0, amp=0.1, w=0.5, phi=0.0):
    """Constant speed along the path, a gentle lateral wave: the six planes [K, n] with their exact derivatives"""
    s0, v0, d0, amp, w, phi = (np.asarray(q, float).reshape(-1, 1) for q in np.broadcast_arrays(s0, v0, d0, amp, w, phi))
    tt = DT * np.arange(n)[None, :]
    return [s0 + v0 * tt, v0 + 0.0 * tt, 0.0 * v0 * tt, d0 + amp * np.sin(w * tt + phi), amp * w * np.cos(w * tt + phi), -amp * w * w * np.sin(w * tt + phi)]


def _swerve(planes, ks):
    """... and trajectories no steering follows"""
    n = planes[0].shape[1]
    tt = DT * np.arange(n)
    for k in ks:
        planes[3][k], planes[4][k], planes[5][k] = 3.0 * np.sin(3.2 * tt), 9.6 * np.cos(3.2 * tt), -30.72 * np.sin(3.2 * tt)
    return planes


def _circle_ahead(p, o, k, j, r=0.02):
    """A small circle the ego rectangle of trajectory k reaches first at pose j >= 1: half a step ahead of where its front was at pose
    j - 1"""
    reach = p.wb_rear_axle + 0.5 * p.length
    fx, fy = o.x[k] + reach * np.cos(o.theta[k]), o.y[k] + reach * np.sin(o.theta[k])
    return [0.5 * (fx[j - 1] + fx[j]), 0.5 * (fy[j - 1] + fy[j]), r]


def _circle_line(t, s_from, s_to, d=LINE_D, r=0.5):
    s = np.arange(s_from, s_to, 2.0 * r)
    x, y, _ = L.points(t, s, np.full(s.shape, d))
    return np.stack((x, y, np.full(s.shape, r)), 1)


def _scatter(rng, p, o, n_static, n_dyn, spread, dyn_t0=0, n_steps=0):
    """Static shapes around poses of kinematically feasible trajectories; dynamic rectangles that follow one of them at the time
    indices of its poses (even obstacles) or of its segments (odd ones), a few metres off, present four steps out of five"""
    feas = np.flatnonzero(o.status == 1)
    def near():
        k = int(rng.choice(feas))
        return k, int(rng.integers(0, o.lengths[k]))

    sobb, tri, circ = [], [], []
    for j in range(n_static):
        k, i = near()
        px, py = o.x[k, i] + rng.normal(0, spread), o.y[k, i] + rng.normal(0, spread)
        if j % 3 == 0:
            sobb.append([px, py, rng.uniform(-3, 3), rng.uniform(0.2, 4.0), rng.uniform(0.05, 1.0)])
        elif j % 3 == 1:
            tri.append([px, py, px + rng.uniform(0.2, 2), py + rng.uniform(-1, 1), px + rng.uniform(-1, 1), py + rng.uniform(0.2, 2)])
        else:
            circ.append([px, py, rng.uniform(0.1, 1.5)])
    dyn = np.full((n_dyn, n_steps, 5), np.nan)
    for j in range(n_dyn):
        k = int(rng.choice(feas))
        off = rng.normal(0, spread, 2)
        for q in range(n_steps):
            if rng.random() < 0.8:
                i = dyn_t0 + q - int(p.time_step0)
                i = i // int(p.factor) if j % 2 == 0 else i
                i = min(max(i, 0), int(o.lengths[k]) - 1)
                dyn[j, q] = (o.x[k, i] + off[0], o.y[k, i] + off[1], rng.uniform(-3, 3), rng.uniform(0.2, 2.5), rng.uniform(0.2, 1.2))
    return ObstacleTables(static_obb=sobb, static_tri=tri, static_circ=circ, dyn_obb=dyn, dyn_t0=dyn_t0)


def _params(p, **changes):
    q = RpParams.from_buffer_copy(p)
    for name, v in changes.items():
        setattr(q, name, v)
    return q


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of one synthetic case and the reference's answer: a namespace with p, cost, path, obs, planes (six [K, n]), lengths,
    theta0, mode, ref"""
    rng = np.random.default_rng([SEED, list(CASES).index(name)])
    f = S.fixture("cfg2_ref_draw")
    t = L.fixture_path("cfg2_ref_draw")
    K, n = CASES[name]
    p, cost, lengths, theta0, mode, obs = f.p, f.cost, None, None, POSES | SWEPT, None
    lift = lambda planes, path=t, params=f.p: L.reference(params, path, *planes, lengths=lengths, theta0=theta0)   # noqa: E731
    if name in ("n63", "n64", "n65", "n129"):
        planes = _cruise(n, 40.0, [5.0, 5.5], [-2.0, 2.0], phi=[0.0, 1.0])
        o = lift(planes)
        targets = {"n63": [(1, 62)], "n64": [(0, 63)], "n65": [(0, 64)], "n129": [(0, 128)]}[name]
        obs = ObstacleTables(static_circ=[_circle_ahead(p, o, k, j) for k, j in targets])
    elif name == "ragged":
        src = L.case("ragged")
        planes, lengths = list(src.planes), src.lengths
        obs = _scatter(rng, p, src.out, 9, 4, 2.0, dyn_t0=1, n_steps=60)
    elif name == "many":
        a_side = np.arange(K) < 1025
        v0 = np.where(a_side, rng.uniform(4.5, 7.0, K), rng.uniform(2.0, 3.0, K))
        v0[:1025:8] = rng.uniform(9.5, 10.0, len(v0[:1025:8]))   # colliding, and costlier than the winner
        d0 = np.where(a_side, rng.uniform(-2.0, -0.5, K), rng.uniform(1.6, 2.0, K))
        planes = _swerve(_cruise(n, rng.uniform(20.0, 60.0, K), v0, d0, phi=rng.uniform(0.0, 6.0, K)), range(1, K, 2))
        obs = ObstacleTables(static_circ=_circle_line(t, 15.0, 90.0))
        mode = POSES
    elif name == "factor3":
        p = _params(f.p, factor=3, time_step0=2)
        planes = _swerve(_cruise(n, 30.0 + 12.0 * np.arange(K), rng.uniform(9.0, 10.0, K), np.linspace(-1.0, 1.0, K), phi=rng.uniform(0.0, 6.0, K)), (3,))
        o = lift(planes, params=p)
        first, n_steps = 3, 24                        # time indices 3 .. 26: behind pose 0 (2), in front of the last segment (2 + 28)
        dyn = np.full((4, n_steps, 5), np.nan)
        at = lambda k, i: (o.x[k, i] + p.wb_rear_axle * np.cos(o.theta[k, i]), o.y[k, i] + p.wb_rear_axle * np.sin(o.theta[k, i]), o.theta[k, i], 0.3, 0.3)   # noqa: E731
        dyn[0, 2 + 3 * 4 - first] = at(0, 4)          # where trajectory 0 is at pose 4, at pose 4's time index 14
        dyn[1, 2 + 10 - first] = at(1, 10)            # where trajectory 1 is at pose 10, at SEGMENT 10's time index 12: no pose has it
        dyn[2, 0] = at(2, 0)                          # where trajectory 2 starts, at index 3: pose 0 has index 2, in front of the table
        dyn[3, n_steps - 1] = at(4, 8)                # where trajectory 4 is at pose 8 (index 26, the table's last): pose 9 has 29, behind it
        obs = ObstacleTables(dyn_obb=dyn, dyn_t0=first)
    elif name == "standstill":
        planes = L._speed_profile(rng, K, n, t.pos[-1] - t.pos[0], [(60, 70)])
        theta0 = np.array([0.5, -0.4, 1.1, 3.0])
        o = lift(planes)
        # A small rectangle present at pose 65's time index alone, at the front corner the KEPT orientation swings the vehicle over.
        # With lon the corner's distance from the rear axle, the rectangle that followed the path instead would have its side lon *
        # |swing| further in: the obstacle sits 0.4 of that inside the vehicle as it stands, 0.6 of it outside the other one.
        dyn = np.full((K, n, 5), np.nan)
        lon, half = p.wb_rear_axle + 0.5 * p.length - 0.05, 0.5 * p.width
        for k in range(0, K, 2):
            th, swing = o.theta[k, 65], o.theta_cl[k, 65]   # (at a standstill theta_cl is the kept orientation minus the path's)
            if abs(swing) < 0.01:
                continue
            lat = math.copysign(half - 0.4 * lon * abs(swing), swing)
            dyn[k, 65] = (o.x[k, 65] + lon * math.cos(th) - lat * math.sin(th), o.y[k, 65] + lon * math.sin(th) + lat * math.cos(th), th, 0.001, 0.001)
        obs = ObstacleTables(dyn_obb=dyn, dyn_t0=int(p.time_step0))
        mode = POSES
    elif name == "low_vel":
        src = L.case("low_vel")
        p, t, planes = src.p, src.path, list(src.planes)
        cost = S.fixture("scurve_lv_l1_draw").cost
        obs = _scatter(rng, p, src.out, 5, 3, 2.5, dyn_t0=int(p.time_step0) + 1, n_steps=n - 4)
    elif name == "long_path":
        src = L.case("long_path")
        t, planes = src.path, list(src.planes)
        obs = _scatter(rng, p, src.out, 6, 3, 2.0, dyn_t0=1, n_steps=n - 4)
    elif name == "many_static":
        planes = _swerve(_cruise(n, rng.uniform(30.0, 60.0, K), rng.uniform(4.0, 7.0, K), np.linspace(-3.0, 3.0, K), phi=rng.uniform(0.0, 6.0, K)), (4,))
        obs = _scatter(rng, p, lift(planes), CK_LDS_ROWS + 1, 0, 45.0)
    elif name == "all_infeasible":
        planes = _swerve(_cruise(n, rng.uniform(30.0, 60.0, K), rng.uniform(4.0, 7.0, K), 0.0), range(K))
        obs = ObstacleTables(static_circ=_circle_line(t, 25.0, 80.0, d=0.0))
    elif name in ("all_collide", "mode0"):
        rng = np.random.default_rng([SEED, 777])      # the same inputs in both
        planes = _swerve(_cruise(n, rng.uniform(30.0, 60.0, K), rng.uniform(4.0, 7.0, K), rng.uniform(-1.8, -0.7, K), phi=rng.uniform(0.0, 6.0, K)), (1, 4))
        obs = ObstacleTables(static_circ=_circle_line(t, 25.0, 85.0))
        mode = 0 if name == "mode0" else POSES | SWEPT
    elif name == "no_obstacles":
        planes = _swerve(_cruise(n, rng.uniform(30.0, 60.0, K), rng.uniform(4.0, 7.0, K), rng.uniform(-2.0, 2.0, K), phi=rng.uniform(0.0, 6.0, K)), (0, 3, 6))
        mode = POSES
    elif name == "duplicates":
        vd = float(cost.desired_speed)
        v0 = np.array([5.0, vd, 5.5, 3.0, 3.2, 5.5, vd, 3.4])
        d0 = np.array([0.0, LINE_D, 1.6, 2.0, 2.0, 1.6, LINE_D, 2.0])
        planes = _swerve(_cruise(n, 40.0, v0, d0, phi=[0.0, 0.3, 0.6, 0.9, 1.2, 0.6, 0.3, 1.5]), (0,))
        obs = ObstacleTables(static_circ=_circle_line(t, 30.0, 60.0))
    else:
        raise KeyError(name)
    planes = tuple(np.ascontiguousarray(q) for q in planes)
    for q in planes:
        q.setflags(write=False)
    c = NS(name=name, p=p, cost=cost, path=t, obs=obs, planes=planes, lengths=lengths, theta0=theta0, mode=mode)
    c.ref = reference(p, cost, t, obs, planes, lengths=lengths, theta0=theta0, mode=mode)
    return c
