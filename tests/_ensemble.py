"""Shared by the tests of tests/test_ensemble_check.py, on the oracle alone and on the device: the cases of the ensemble
checker (include/rp_ensemble.h), their members and the oracle's verdicts on them.  Expected values come only from
``oracle.check_poses`` and ``oracle.check_swept``, run per (trajectory, member) with ``OracleTables`` built from that member's table;
they are computed once per session and never written to."""
import functools
import os
import re

import numpy as np

from commonroad_rp_amd.collision import ObstacleTables
from test_trajectory_check import LDS_ROWS as CHECKER_LDS_ROWS
from test_trajectory_check import WB, _oracle_batch, _params, _random_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rp_ensemble.h")
SOURCE = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_ensemble.hip")
_SRC = open(SOURCE).read() if os.path.exists(SOURCE) else ""


def _constant(name, default):
    m = re.search(rf"\b{name}\s*=\s*(\d+)\s*;", _SRC)
    return int(m.group(1)) if m else default


LDS_ROWS = _constant("EN_LDS_ROWS", CHECKER_LDS_ROWS)   # static rows the kernel stages in LDS; beyond: read from device memory
MEMBER_BLOCK = _constant("EN_MEMBER_BLOCK", 0)          # members one wavefront walks; 0: the kernel has no member block
SEED = 2025

# (K, n_poses, n_dyn, n_static, factor, ragged lengths, scatter of the static shapes around the poses [m], of the dynamic obstacles, M)
CASES = [
    (1, 130, 5, 6, 1, False, 3.0, 3.0, 3),
    (2, 65, 1, 0, 3, True, 1.0, 1.0, 2),
    (63, 3, 0, 6, 1, True, 5.0, 5.0, 4),
    (64, 64, 9, 0, 1, False, 8.0, 8.0, 5),
    (65, 63, 5, LDS_ROWS + 1, 3, True, 60.0, 4.0, 17),
    (5, 1, 5, 3, 1, False, 3.0, 3.0, 1),
    (9, 70, 6, 3, 2, True, 40.0, 3.0, 8),
    (257, 2, 1, 6, 1, True, 5.0, 5.0, 2),
] + [(9, 70, 6, 3, 1, True, 40.0, 3.0, M) for M in ((MEMBER_BLOCK - 1, MEMBER_BLOCK, MEMBER_BLOCK + 1) if MEMBER_BLOCK > 1 else (1, 2, 3))]
N130, NO_DYN, SPREAD_5, SPREAD_17, ONE_MEMBER, N70 = 0, 2, 3, 4, 5, 6
DEVICE_MEMORY_CASE = SPREAD_17   # more static shapes than the LDS copy holds
MEMBER_SIGMA = 2.0               # metres


def make_members(rng, dyn):
    """The member recipe: member 0 is the table itself; in member m > 0 every obstacle's track is shifted in x and y by one
    N(0, 2 m) draw per (member, obstacle); every member with m % 3 == 2 loses one whole obstacle (its rows become NaN)."""
    def recipe(M):
        out = np.repeat(dyn[None], M, axis=0)
        for m in range(1, M):
            out[m, :, :, 0:2] += rng.normal(0.0, MEMBER_SIGMA, (dyn.shape[0], 1, 2))
            if m % 3 == 2 and dyn.shape[0]:
                out[m, rng.integers(0, dyn.shape[0])] = np.nan
        return out
    return recipe


def static_only(obs):
    return ObstacleTables(static_obb=obs.static_obb, static_tri=obs.static_tri, static_circ=obs.static_circ)


def with_member(obs, table, dyn_t0):
    return ObstacleTables(static_obb=obs.static_obb, static_tri=obs.static_tri, static_circ=obs.static_circ, dyn_obb=table, dyn_t0=dyn_t0)


def oracle_ensemble(p, obs, members, dyn_t0, x, y, th, lengths):
    """(first_pose_hit [K, M], first_segment_hit [K, M]) of the oracle: member by member, trajectory by trajectory."""
    K, M = x.shape[0], members.shape[0]
    first_pose, first_seg = np.empty((K, M), np.int32), np.empty((K, M), np.int32)
    for m in range(M):
        first_pose[:, m], _, first_seg[:, m] = _oracle_batch(p, with_member(obs, members[m], dyn_t0), x, y, th, lengths)
    return first_pose, first_seg


def members_hit(first_pose, first_seg, poses, swept):
    hit = np.zeros(first_pose.shape, bool)
    if poses:
        hit |= first_pose >= 0
    if swept:
        hit |= first_seg >= 0
    return hit.sum(axis=1).astype(np.int32)


def first_free_and_n_over(count, max_members_hit):
    free = np.flatnonzero(count <= max_members_hit)
    return (int(free[0]) if len(free) else -1), int((count > max_members_hit).sum())


class Case:
    """x, y, th [K, n], lengths [K] or None, p (rp_params), obs (static shapes and member 0 as its dynamic table), members
    [M, n_dyn, n_steps, 5], dyn_t0, and the oracle's first_pose, first_seg [K, M]."""

    def freeze(self):
        for a in (self.x, self.y, self.th, self.members, self.first_pose, self.first_seg):
            a.setflags(write=False)
        return self

    @property
    def M(self):
        return self.members.shape[0]


@functools.lru_cache(maxsize=None)
def cases():
    """The random batches, their members and the oracle's verdicts on them: computed once, read by every test."""
    rng = np.random.default_rng(SEED)
    out = []
    for K, n, n_dyn, n_static, factor, ragged, scatter, dyn_scatter, M in CASES:
        c = Case()
        c.x, c.y, c.th, c.lengths, t0, c.obs = _random_batch(rng, K, n, n_dyn, n_static, ragged, scatter, dyn_scatter)
        c.members, c.dyn_t0 = make_members(rng, c.obs.dyn_obb)(M), c.obs.dyn_t0
        c.p = _params(time_step0=t0, factor=factor, n=n)
        c.first_pose, c.first_seg = oracle_ensemble(c.p, c.obs, c.members, c.dyn_t0, c.x, c.y, c.th, c.lengths)
        out.append(c.freeze())
    return out


def _boundary_scene(n, plan, extra_static=0):
    """Hits on both sides of a wavefront's boundary ACROSS THE MEMBERS, by construction.  Every trajectory drives straight along x,
    12 m per step -- consecutive rectangles leave gaps -- 100 m beside the next one.  plan[k][m]: the pose of trajectory k on which
    member m has a small dynamic rectangle, present at that pose's time index only (-1: none in this member): pose i and segment i
    meet it there.  plan[k] may end in ("static", i): a disc on pose i, met by pose i and segments i - 1 and i in every member."""
    t0, r = 3, 0.2
    K = len(plan)
    M = max(len([q for q in row if not isinstance(q, tuple)]) for row in plan)
    x = np.tile(12.0 * np.arange(n), (K, 1))
    y = np.tile(100.0 * np.arange(K)[:, None], (1, n))
    th = np.zeros((K, n))
    members = np.full((M, K, n + 4, 5), np.nan)
    circ = []
    for k, row in enumerate(plan):
        for m, i in enumerate(q for q in row if not isinstance(q, tuple)):
            if i >= 0:
                members[m, k, t0 + i] = (x[k, i] + WB, y[k, 0], 0.0, r, r)
        circ += [[x[k, q[1]] + WB, y[k, 0], r] for q in row if isinstance(q, tuple)]
    circ += [[-1e4 - 10.0 * j, -1e4, 1.0] for j in range(extra_static)]   # far away: they only fill the table
    c = Case()
    c.x, c.y, c.th, c.lengths = x, y, th, None
    c.obs, c.members, c.dyn_t0 = ObstacleTables(static_circ=circ, dyn_obb=members[0], dyn_t0=0), members, 0
    c.p = _params(time_step0=t0, n=n)
    c.first_pose, c.first_seg = oracle_ensemble(c.p, c.obs, c.members, c.dyn_t0, c.x, c.y, c.th, c.lengths)
    # what the construction aims at: the member's own pose, or the static disc where that comes first
    c.aim_pose = np.full((K, M), -1, np.int32)
    c.aim_seg = np.full((K, M), -1, np.int32)
    for k, row in enumerate(plan):
        stat = [q[1] for q in row if isinstance(q, tuple)]
        for m, i in enumerate(q for q in row if not isinstance(q, tuple)):
            poses = [q for q in [i] + stat if q >= 0]
            segs = [q for q in [i] + stat + [s - 1 for s in stat] if 0 <= q < n - 1]
            c.aim_pose[k, m] = min(poses) if poses else -1
            c.aim_seg[k, m] = min(segs) if segs else -1
    return c.freeze()


BOUNDARY_PLAN_130 = [
    [62, 63, 64, 65],            # one trajectory, first hits on both sides of 63 | 64 across its members
    [64, 63, 128, -1],
    [127, 128, 129, 5],
    [-1, 64, -1, 63],
    [100, 20, 64, 129, ("static", 64)],   # the static disc caps every member: 64, 20, 64, 64
    [-1, -1, -1, -1, ("static", 63)],     # static alone, the same in every member
    [-1, -1, -1, -1],            # free in every member
]
BOUNDARY_PLAN_70 = [
    [62, 63, 64, 69],
    [64, 0, -1, 63],
    [-1, -1, 68, -1, ("static", 65)],
    [-1, -1, -1, -1],
]


@functools.lru_cache(maxsize=None)
def boundary_cases():
    return [_boundary_scene(130, BOUNDARY_PLAN_130), _boundary_scene(70, BOUNDARY_PLAN_70),
            _boundary_scene(130, BOUNDARY_PLAN_130, extra_static=LDS_ROWS)]
