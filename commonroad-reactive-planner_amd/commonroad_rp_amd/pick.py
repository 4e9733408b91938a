"""The cheapest feasible, collision-free one of curvilinear trajectories the caller brings: ctypes binding of ``include/rp_pick.h``
(``librp_pick.so``, built from ``csrc/rp_pick.hip``).

``TrajectoryLifter`` lifts given trajectories s, s', s'', d, d', d'', ``TrajectoryScorer`` prices given poses and ``TrajectoryChecker``
checks them; a caller who wanted ``ReactivePlanner._get_optimal_trajectory`` for such a bundle chained the three through host memory.
``TrajectoryPicker`` is that decision in one device round trip: per trajectory the status word, the default cost and the first
colliding pose / segment, per call the cheapest kinematically feasible and collision-free trajectory, the reference planner's
statistics and the winner's state block.  No pose plane comes back to the host unless it is asked for.  A ``TrajectoryPicker`` shares
nothing with an ``RpContext``, the lifter, the checkers or the scorer.  There is NO CPU fallback: without the library creating one
raises ``RpLibraryMissing``, without a GPU ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpCost, RpParams, dptr
from ._session import as_ip

__all__ = ["TrajectoryPicker", "TrajectoryPickResult", "RpPickResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_pick.so")
ABI_VERSION = 1
TRAJ_POSES, TRAJ_SWEPT = 1, 2
MAX_POSES = 1 << 24
RP_N_ARRAYS = 14
PLANES = ("x", "y", "theta", "v", "a", "kappa", "kappa_dot", "theta_cl")


class RpPickResult(C.Structure):
    """``rp_pick_result`` of include/rp_pick.h"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("best", C.c_int64), ("best_cost", C.c_double), ("n_feasible", C.c_int64),
                ("n_collision", C.c_int64), ("n_collision_before_best", C.c_int64), ("reason_counts", C.c_int64 * 8)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(type(self))


_dp, _ip, _up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
_SIGNATURES = {
    "rp_pick_abi_version": (C.c_int, []),
    "rp_pick_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_pick_destroy": (None, [C.c_void_p]),
    "rp_pick_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_pick_set_reference": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_double]),
    "rp_pick_set_obstacles": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "rp_pick_select": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.POINTER(RpCost), C.c_uint32, C.c_int64, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp,
                                 _ip, _dp, C.c_uint32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _up, _dp, _ip, _ip, C.POINTER(RpPickResult), _dp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_pick.so`` and declare every entry point of ``include/rp_pick.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


@dataclasses.dataclass
class TrajectoryPickResult:
    """``status``: [K] uint32, label | reason << 4 | step << 8 (``RP_STATUS_*`` of include/rp_amd.h; label 1 feasible and free, 2
    kinematically infeasible, 3 feasible but colliding -- then ``step`` is the first colliding pose, or segment if only that test hit);
    ``cost``: [K] float64, NaN for a kinematically infeasible trajectory; ``best``: the cheapest trajectory with label 1 (ties: the
    smaller index) or -1, ``best_cost`` its cost or NaN, ``best_states``: its [14, n] state block in the row layout of
    ``RpContext.fetch_states()`` or None; ``n_feasible``: kinematically feasible trajectories, colliding ones included; ``n_collision``:
    those with a hit; ``n_collision_before_best``: those of them cheaper than the winner (all, without one); ``reason_counts``: [8] int64,
    trajectories per kinematic reason code; ``x`` .. ``theta_cl``: [K, n] float64 or None (``want_planes``); ``first_pose_hit`` /
    ``first_segment_hit``: [K] int32, -1 where nothing hit and where the trajectory was not tested, or None (``want_hits`` and the
    test)."""
    status: np.ndarray
    cost: np.ndarray
    best: int
    best_cost: float
    best_states: Optional[np.ndarray]
    n_feasible: int
    n_collision: int
    n_collision_before_best: int
    reason_counts: np.ndarray
    x: Optional[np.ndarray] = None
    y: Optional[np.ndarray] = None
    theta: Optional[np.ndarray] = None
    v: Optional[np.ndarray] = None
    a: Optional[np.ndarray] = None
    kappa: Optional[np.ndarray] = None
    kappa_dot: Optional[np.ndarray] = None
    theta_cl: Optional[np.ndarray] = None
    first_pose_hit: Optional[np.ndarray] = None
    first_segment_hit: Optional[np.ndarray] = None

    @property
    def label(self) -> np.ndarray:
        return self.status & 3

    @property
    def reason(self) -> np.ndarray:
        return (self.status >> 4) & 7

    @property
    def step(self) -> np.ndarray:
        return (self.status >> 8) & 0xFFF


class TrajectoryPicker(_session.Session):
    """Owner of one ``rp_pick`` (one HIP stream, the segment table of one reference path, obstacle tables, input and result buffers)."""

    _prefix, _load = "rp_pick", staticmethod(load_library)

    def set_reference(self, ref_xy, ref_pos=None, ref_theta=None, ref_curv=None, ref_curv_d=None, d_limit: Optional[float] = None):
        """The arguments of ``TrajectoryLifter.set_reference``: the tables of ``rp_build_reference`` -- vertices [n, 2], arc lengths,
        unwrapped orientations, curvature and its derivative, [n] each -- or the package's ``CoordinateSystem`` alone (its
        projection-domain limit unless ``d_limit`` is given).  Replaces the earlier table."""
        self._set_reference(ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, d_limit)

    def set_obstacles(self, tables=None):
        """The tables ``RpContext.set_obstacles`` takes (``ObstacleTables``; None: empty); they replace the earlier ones."""
        self._set_obstacles(tables)

    def pick(self, params: RpParams, cost: RpCost, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=None, theta0=None, poses: bool = True,
             swept: bool = False, want_planes: bool = False, want_hits: bool = False) -> TrajectoryPickResult:
        """The six planes: [K, n] (one trajectory may come as 1-D); ``lengths``: [K] valid poses per trajectory (None: n); ``theta0``:
        [K] orientations the trajectories start with (None: ``params.x0_orientation``).  ``poses``: the per-pose collision test at time
        index ``time_step0 + i * factor``; ``swept``: the continuous test of segment i at ``time_step0 + i``; neither: no collision test.
        ``want_planes``: the eight pose planes come back (otherwise none of them leaves the device); ``want_hits``: the first-hit arrays
        of the requested tests come back.  ``params``, ``cost``: what ``_capi.make_params`` and ``_capi.make_cost`` return."""
        s, s_dot, s_ddot, d, d_dot, d_ddot = _session.six_planes("pick", s, s_dot, s_ddot, d, d_dot, d_ddot)
        K, n = s.shape
        lens, th0 = _session.lengths_of("pick", lengths, K), _session.theta0_of("pick", theta0, K)
        mode = (TRAJ_POSES if poses else 0) | (TRAJ_SWEPT if swept else 0)
        planes = [np.empty((K, n)) if want_planes else None for _ in PLANES]
        status, costs = np.empty(K, dtype=np.uint32), np.empty(K)
        first_pose = np.empty(K, dtype=np.int32) if want_hits and poses else None
        first_seg = np.empty(K, dtype=np.int32) if want_hits and swept else None
        res = RpPickResult()
        block = np.empty((RP_N_ARRAYS, n))
        self._call("select", C.byref(params), C.byref(cost), mode, K, n, dptr(s), dptr(s_dot), dptr(s_ddot), dptr(d), dptr(d_dot), dptr(d_ddot),
                   as_ip(lens), dptr(th0), 0, *[dptr(q) for q in planes], status.ctypes.data_as(_up), dptr(costs), as_ip(first_pose), as_ip(first_seg),
                   C.byref(res), dptr(block))
        return TrajectoryPickResult(status, costs, int(res.best), float(res.best_cost), block if res.best >= 0 else None, int(res.n_feasible),
                                    int(res.n_collision), int(res.n_collision_before_best), np.array(res.reason_counts[:], dtype=np.int64),
                                    *planes, first_pose, first_seg)
