"""Shared by tests/test_epick_abi.py (CPU) and tests/test_epick.py (GPU): the yardstick of the pick under a risk bound
(include/rp_epick.h).  A composition, nothing restated --

  ``_lift.reference``                      the eight planes and the kinematic status word,
  ``_score.cost_of``                       the cost,
  ``_pick.first_hits``                     the first colliding pose / segment, per member on ``_ensemble.with_member``'s tables,
  a plain Python loop over ascending m     the risk,
  ``_pick.select``                         the winner and the collisions in front of it.

The cases take the inputs of ``_pick.case`` and ``_pick.pin`` and add members by ``_ensemble.make_members``.  What does not depend on
the weights and the bound (lift, cost, first hits) is computed once per case and never written to; ``decide`` puts weights and a bound
on it."""
import functools
import math
import os
import re
from types import SimpleNamespace as NS

import numpy as np

from commonroad_rp_amd.collision import ObstacleTables

import _ensemble as E
import _lift as L
import _pick as P
import _score as S

REPO = S.REPO
HEADER = os.path.join(REPO, "include", "rp_epick.h")
CSRC = P.CSRC
SOURCE = os.path.join(CSRC, "rp_epick.hip")
_SRC = open(SOURCE).read() if os.path.exists(SOURCE) else ""


def _constant(name, default):
    m = re.search(rf"\b{name}\s*=\s*(\d+)\s*;", _SRC)
    return int(m.group(1)) if m else default


LF_LDS_ROWS = _constant("EP_LF_LDS_ROWS", 384)     # segment rows the lift kernel stages in LDS
CK_LDS_ROWS = _constant("EP_CK_LDS_ROWS", 128)     # static shapes the collision kernel stages in LDS
MEMBER_BLOCK = _constant("EP_MEMBER_BLOCK", 1)     # members one wavefront of the collision kernel walks
POSES, SWEPT = P.POSES, P.SWEPT
SEED = 7


# ---- the reference -------------------------------------------------------------------------------------------------------------
def member_hits(p, t, obs, members, dyn_t0, o, mode, grow=0.0):
    """(first_pose_hit, first_segment_hit), [K, M] int32 each: ``_pick.first_hits`` member by member"""
    obs = obs if obs is not None else ObstacleTables()
    K, M = len(o.status), members.shape[0]
    fp, fs = np.empty((K, M), np.int32), np.empty((K, M), np.int32)
    for m in range(M):
        fp[:, m], fs[:, m] = P.first_hits(p, t, E.with_member(obs, members[m], dyn_t0), o, mode, grow=grow)
    return fp, fs


def risk_of(hit, weights, order=None):
    """sum of weights[m] over the members with a hit, in double, one after the other from 0.0, in ascending m (or in ``order``)"""
    K, M = hit.shape
    out = np.zeros(K)
    for k in range(K):
        r = 0.0
        for m in (range(M) if order is None else order):
            if hit[k, m]:
                r = r + float(weights[m])
        out[k] = r
    return out


def base(p, cost, t, obs, members, dyn_t0, planes, lengths=None, theta0=None, mode=POSES):
    """What does not depend on weights and bound: lift, cost [K], first_pose_hit, first_segment_hit [K, M], hit [K, M], members_hit [K]"""
    planes = [np.atleast_2d(np.asarray(q, float)) for q in planes]
    o = L.reference(p, t, *planes, lengths=lengths, theta0=theta0)
    K = planes[0].shape[0]
    costs = np.full(K, np.nan)
    for k in np.flatnonzero(o.status == 1):
        m = int(o.lengths[k])
        costs[k] = S.cost_of(cost, o.a[k, :m], o.v[k, :m], planes[0][k, :m], planes[3][k, :m], o.theta_cl[k, :m])
    fp, fs = member_hits(p, t, obs, members, dyn_t0, o, mode)
    hit = (fp >= 0) | (fs >= 0)
    for a in (costs, fp, fs, hit):
        a.setflags(write=False)
    return NS(lift=o, planes=planes, cost=costs, first_pose_hit=fp, first_segment_hit=fs, hit=hit, members_hit=hit.sum(axis=1).astype(np.int32))


def decide(b, weights=None, max_risk=0.0):
    """What rp_epick_select returns on the case behind ``b``, as a namespace: the fields of ``_pick.reference`` (first hits [K, M]) and
    members_hit, risk [K], best_members_hit, best_risk"""
    o = b.lift
    K, M = b.hit.shape
    n = b.planes[0].shape[1]
    w = np.ones(M) if weights is None else np.asarray(weights, float)
    risk = risk_of(b.hit, w)
    status = o.status.copy()
    for k in np.flatnonzero((o.status == 1) & (risk > max_risk)):
        fp, fs = b.first_pose_hit[k], b.first_segment_hit[k]
        step = fp[fp >= 0].min() if (fp >= 0).any() else fs[fs >= 0].min()
        status[k] = S.status_word(3, 0, min(int(step), 0xFFF))
    best, before = P.select(status, b.cost)
    block = None
    if best >= 0:
        block = np.full((14, n), np.nan)
        m = int(o.lengths[best])
        for row, name in zip(P.PLANE_ROWS, L.PLANES):
            block[row] = getattr(o, name)[best]
        for row, q in zip(P.INPUT_ROWS, b.planes):
            block[row, :m] = q[best, :m]
    return NS(lift=o, status=status, cost=b.cost, first_pose_hit=b.first_pose_hit, first_segment_hit=b.first_segment_hit, members_hit=b.members_hit,
              risk=risk, best=best, best_cost=b.cost[best] if best >= 0 else math.nan, best_states=block, n_feasible=int((o.status == 1).sum()),
              n_collision=int(((status & 3) == 3).sum()), n_collision_before_best=before, reason_counts=o.reason_counts,
              best_members_hit=int(b.members_hit[best]) if best >= 0 else -1, best_risk=float(risk[best]) if best >= 0 else math.nan)


def steady(c):
    """Every first hit per member unchanged with the vehicle ``_pick.EDGE`` longer and wider and EDGE shorter and narrower"""
    ok = True
    for grow in (P.EDGE, -P.EDGE):
        fp, fs = member_hits(c.p, c.path, c.obs, c.members, c.dyn_t0, c.base.lift, c.mode, grow=grow)
        ok = ok and np.array_equal(fp, c.base.first_pose_hit) and np.array_equal(fs, c.base.first_segment_hit)
    return ok


def cost_gap(c, r):
    """Smallest relative distance of another kinematically feasible trajectory's cost to the winner's of ``r`` (inf without one)"""
    if r.best < 0:
        return math.inf
    others = [k for k in np.flatnonzero(r.lift.status == 1) if k != r.best]
    return min((abs(r.cost[k] - r.best_cost) / abs(r.best_cost) for k in others), default=math.inf)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _empty_members(M=1):
    return np.full((M, 0, 0, 5), np.nan)


def _finish(src, name, members, dyn_t0):
    members = np.ascontiguousarray(members, dtype=float)
    members.setflags(write=False)
    c = NS(name=name, p=src.p, cost=src.cost, path=src.path, obs=src.obs, planes=src.planes, lengths=src.lengths, theta0=src.theta0, mode=src.mode,
           members=members, dyn_t0=dyn_t0, M=members.shape[0])
    c.base = base(c.p, c.cost, c.path, c.obs, members, dyn_t0, c.planes, lengths=c.lengths, theta0=c.theta0, mode=c.mode)
    return c


@functools.lru_cache(maxsize=None)
def single(name):
    """``_pick.case(name)`` (or the pin for "pin") as a case of one member: the case's own dynamic table"""
    src = P.pin() if name == "pin" else P.case(name)
    obs = src.obs if src.obs is not None else ObstacleTables()
    return _finish(src, src.name, obs.dyn_obb[None], int(obs.dyn_t0))


# name -> (the case of tests/_pick.py it takes its inputs from, M)
MULTI = {"long_path_m5": ("long_path", 5), "factor3_m3": ("factor3", 3), "ragged_m9": ("ragged", 9), "long_path_m65": ("long_path", 65)}


@functools.lru_cache(maxsize=None)
def multi(name):
    """The inputs and static shapes of a ``_pick`` case, its dynamic table as member 0 of M by ``_ensemble.make_members``"""
    source, M = MULTI[name]
    src = P.case(source)
    rng = np.random.default_rng([SEED, M])
    return _finish(src, name, E.make_members(rng, src.obs.dyn_obb)(M), int(src.obs.dyn_t0))


# where the boundary case puts its rectangles: (trajectory, member, pose it sits on, "pose" or "segment": whose time index it has)
BOUNDARY_N = 80


BOUNDARY_BLOCK = max(MEMBER_BLOCK, 2)   # (with a block of one member every member is a block's first and last)


def boundary_plan():
    B = BOUNDARY_BLOCK
    return [(0, 0, 63, "pose"), (0, B - 1, 64, "pose"), (0, B, 64, "pose"), (0, 2 * B - 1, 63, "pose"),
            (1, 0, 64, "segment"), (1, B - 1, 70, "segment"), (1, 2 * B - 1, 62, "segment")]


@functools.lru_cache(maxsize=None)
def boundary():
    """Four trajectories of 80 poses, factor 3, two member blocks.  A small rectangle placed as ``_pick.case("factor3")`` places its
    own -- on the ego rectangle of one pose, present at one time index -- sits on pose 63 in one member and on pose 64 in another
    (both sides of a wavefront's boundary), in the first and the last member of each member block, and on poses 64, 70 and 62 at the
    time index of the SEGMENT that starts there, which no pose has.  Trajectory 2 is free in every member, trajectory 3 infeasible."""
    f = S.fixture("cfg2_ref_draw")
    t = L.fixture_path("cfg2_ref_draw")
    K, n, M = 4, BOUNDARY_N, 2 * BOUNDARY_BLOCK
    p = P._params(f.p, factor=3, time_step0=2)
    planes = P._swerve(P._cruise(n, 30.0 + 12.0 * np.arange(K), [5.0, 5.2, 5.4, 5.0], np.linspace(-1.5, 1.5, K), phi=[0.0, 1.0, 2.0, 3.0]), (3,))
    o = L.reference(p, t, *planes)
    first, n_steps = 3, 3 * n
    members = np.full((M, K, n_steps, 5), np.nan)
    at = lambda k, i: (o.x[k, i] + p.wb_rear_axle * np.cos(o.theta[k, i]), o.y[k, i] + p.wb_rear_axle * np.sin(o.theta[k, i]), o.theta[k, i], 0.3, 0.3)   # noqa: E731
    for k, m, i, kind in boundary_plan():
        index = int(p.time_step0) + (3 * i if kind == "pose" else i)
        members[m, k, index - first] = at(k, i)
    planes = tuple(np.ascontiguousarray(q) for q in planes)
    for q in planes:
        q.setflags(write=False)
    src = NS(name="boundary", p=p, cost=f.cost, path=t, obs=ObstacleTables(), planes=planes, lengths=None, theta0=None, mode=POSES | SWEPT)
    return _finish(src, "boundary", members, first)
