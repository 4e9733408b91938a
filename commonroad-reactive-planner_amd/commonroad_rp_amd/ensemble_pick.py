"""The cheapest feasible one of curvilinear trajectories the caller brings whose collision risk over M sampled predictions stays under
a bound: ctypes binding of ``include/rp_epick.h`` (``librp_epick.so``, built from ``csrc/rp_epick.hip``).

``TrajectoryPicker`` decides against ONE table of dynamic obstacles; ``EnsembleChecker`` tests given poses against M sampled futures of
them (the "members") and knows nothing of feasibility or cost.  A caller who plans against uncertain predictions chained the two
through host memory and summed the member weights in NumPy.  ``EnsemblePicker`` is that decision in one device round trip: per
trajectory the status word, the default cost, the members it collides in, the sum of their weights (the risk) and per member the first
colliding pose / segment, per call the cheapest kinematically feasible trajectory with ``risk <= max_risk``, the statistics of
``TrajectoryPicker`` and the winner's state block, member count and risk.  No pose plane comes back to the host unless it is asked
for.  An ``EnsemblePicker`` shares nothing with an ``RpContext`` or the other libraries' objects.  There is NO CPU fallback: without
the library creating one raises ``RpLibraryMissing``, without a GPU ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpCost, RpParams, dptr, f64
from ._session import as_ip

__all__ = ["EnsemblePicker", "EnsemblePickResult", "RpEpickResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_epick.so")
ABI_VERSION = 1
TRAJ_POSES, TRAJ_SWEPT = 1, 2
MAX_MEMBERS = 4096
MAX_DYN_ROWS = 1 << 22
MAX_POSES = 1 << 24
MAX_VERDICTS = 1 << 24
RP_N_ARRAYS = 14
PLANES = ("x", "y", "theta", "v", "a", "kappa", "kappa_dot", "theta_cl")


class RpEpickResult(C.Structure):
    """``rp_epick_result`` of include/rp_epick.h"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("best", C.c_int64), ("best_cost", C.c_double), ("n_feasible", C.c_int64),
                ("n_collision", C.c_int64), ("n_collision_before_best", C.c_int64), ("reason_counts", C.c_int64 * 8),
                ("best_members_hit", C.c_int64), ("best_risk", C.c_double)]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(type(self))


_dp, _ip, _up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
_SIGNATURES = {
    "rp_epick_abi_version": (C.c_int, []),
    "rp_epick_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_epick_destroy": (None, [C.c_void_p]),
    "rp_epick_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_epick_set_reference": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_double]),
    "rp_epick_set_static": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp]),
    "rp_epick_set_members": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp]),
    "rp_epick_select": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.POINTER(RpCost), C.c_uint32, C.c_double, C.c_int64, C.c_int32, _dp, _dp, _dp, _dp, _dp,
                                  _dp, _ip, _dp, C.c_uint32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _up, _dp, _ip, _dp, _ip, _ip,
                                  C.POINTER(RpEpickResult), _dp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_epick.so`` and declare every entry point of ``include/rp_epick.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


@dataclasses.dataclass
class EnsemblePickResult:
    """The fields of ``TrajectoryPickResult`` with these differences: label 3 in ``status`` means kinematically feasible with
    ``risk > max_risk`` (``step``: the smallest first colliding pose over the members, or segment if no member has a pose hit);
    ``n_collision`` counts those; ``first_pose_hit`` / ``first_segment_hit`` are [K, M] int32, one column per member.  Besides:
    ``members_hit``: [K] int32, members in which the trajectory has a hit in a requested test; ``risk``: [K] float64, the sum of their
    weights in ascending member order (both 0 for a kinematically infeasible trajectory); ``best_members_hit`` / ``best_risk``: the
    winner's, -1 and NaN without one."""
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
    members_hit: Optional[np.ndarray] = None
    risk: Optional[np.ndarray] = None
    best_members_hit: int = -1
    best_risk: float = float("nan")

    @property
    def label(self) -> np.ndarray:
        return self.status & 3

    @property
    def reason(self) -> np.ndarray:
        return (self.status >> 4) & 7

    @property
    def step(self) -> np.ndarray:
        return (self.status >> 8) & 0xFFF


class EnsemblePicker(_session.Session):
    """Owner of one ``rp_epick`` (one HIP stream, the segment table of one reference path, static shapes, member tables and weights,
    input and result buffers)."""

    _prefix, _load = "rp_epick", staticmethod(load_library)

    def __init__(self, device: int = 0, library: Optional[str] = None):
        super().__init__(device, library)
        self.n_members = 1

    def set_reference(self, ref_xy, ref_pos=None, ref_theta=None, ref_curv=None, ref_curv_d=None, d_limit: Optional[float] = None):
        """The arguments of ``TrajectoryPicker.set_reference``: the tables of ``rp_build_reference`` or the package's
        ``CoordinateSystem`` alone.  Replaces the earlier table."""
        self._set_reference(ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, d_limit)

    def set_static(self, obs=None):
        """The static shapes of an ``ObstacleTables`` (None: none); they replace the earlier ones, the members stay."""
        self._set_static(obs)

    def set_members(self, members, dyn_t0: int = 0, weights=None):
        """``members``: [M, n_dyn, n_steps, 5] dynamic rectangles (rows of ``ObstacleTables.dyn_obb``, cx = NaN: absent) for scenario
        time steps ``dyn_t0 ..``; ``weights``: [M] what each member adds to the risk of a trajectory that collides in it (None: 1.0
        each).  They replace the earlier members and weights, the static shapes stay; a refused call leaves the earlier ones."""
        mem, M, nd, ns = _session.members_args(members)
        w = None
        if weights is not None:
            w = f64(weights).reshape(-1)
            if w.shape[0] != M:
                raise ValueError(f"set_members: {w.shape[0]} weights for {M} members")
        self._call("set_members", M, nd, ns, int(dyn_t0), dptr(mem) if mem.size else None, dptr(w))
        self.n_members = M

    def pick(self, params: RpParams, cost: RpCost, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=None, theta0=None, poses: bool = True,
             swept: bool = False, max_risk: float = 0.0, want_planes: bool = False, want_hits: bool = False) -> EnsemblePickResult:
        """The six planes, ``lengths``, ``theta0``, ``poses``, ``swept``, ``want_planes`` and ``params``, ``cost`` as in
        ``TrajectoryPicker.pick``; ``max_risk``: the bound (``inf`` accepts everything kinematically feasible); ``want_hits``: the
        [K, M] first-hit matrices of the requested tests come back."""
        s, s_dot, s_ddot, d, d_dot, d_ddot = _session.six_planes("pick", s, s_dot, s_ddot, d, d_dot, d_ddot)
        K, n = s.shape
        M = self.n_members
        lens, th0 = _session.lengths_of("pick", lengths, K), _session.theta0_of("pick", theta0, K)
        mode = (TRAJ_POSES if poses else 0) | (TRAJ_SWEPT if swept else 0)
        planes = [np.empty((K, n)) if want_planes else None for _ in PLANES]
        status, costs = np.empty(K, dtype=np.uint32), np.empty(K)
        members_hit, risk = np.empty(K, dtype=np.int32), np.empty(K)
        first_pose = np.empty((K, M), dtype=np.int32) if want_hits and poses else None
        first_seg = np.empty((K, M), dtype=np.int32) if want_hits and swept else None
        res = RpEpickResult()
        block = np.empty((RP_N_ARRAYS, n))
        self._call("select", C.byref(params), C.byref(cost), mode, float(max_risk), K, n, dptr(s), dptr(s_dot), dptr(s_ddot), dptr(d), dptr(d_dot),
                   dptr(d_ddot), as_ip(lens), dptr(th0), 0, *[dptr(q) for q in planes], status.ctypes.data_as(_up), dptr(costs), as_ip(members_hit),
                   dptr(risk), as_ip(first_pose), as_ip(first_seg), C.byref(res), dptr(block))
        return EnsemblePickResult(status, costs, int(res.best), float(res.best_cost), block if res.best >= 0 else None, int(res.n_feasible),
                                  int(res.n_collision), int(res.n_collision_before_best), np.array(res.reason_counts[:], dtype=np.int64),
                                  *planes, first_pose, first_seg, members_hit, risk, int(res.best_members_hit), float(res.best_risk))
