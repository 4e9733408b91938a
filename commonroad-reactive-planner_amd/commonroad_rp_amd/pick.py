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
import os
import sys
from typing import Optional

import numpy as np

from ._capi import RpCost, RpError, RpLibraryMissing, RpParams, dptr, f64

__all__ = ["TrajectoryPicker", "TrajectoryPickResult", "RpPickResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "librp_pick.so")
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

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_pick.so`` and declare every entry point of ``include/rp_pick.h``."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    # one HIP runtime per process, torch's when it is installed (see _capi.load_library, same switch)
    if "torch" not in sys.modules and not os.environ.get("RP_AMD_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise RpLibraryMissing(
            f"{path} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
            f"or make -C commonroad-reactive-planner_amd/csrc). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.rp_pick_abi_version() != ABI_VERSION:
        raise RpError(f"{path}: ABI version {lib.rp_pick_abi_version()}, this binding speaks {ABI_VERSION}")
    if path == LIB_PATH:
        _lib = lib
    return lib


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


def _plane(a, shape, name):
    a = np.atleast_2d(f64(a)) if np.ndim(a) != 2 else f64(a)
    if a.shape != shape:
        raise ValueError(f"pick: {name} of shape {a.shape}, s of shape {shape}")
    return a


class TrajectoryPicker:
    """Owner of one ``rp_pick`` (one HIP stream, the segment table of one reference path, obstacle tables, input and result buffers)."""

    def __init__(self, device: int = 0, library: Optional[str] = None):
        self._lib = load_library(library)
        self._h = C.c_void_p()
        rc = self._lib.rp_pick_create(C.byref(self._h), int(device))
        if rc != 0:
            msg = self._lib.rp_pick_last_error(self._h) if self._h else b"rp_pick_create failed"
            self.close()
            raise RpError(f"rp_pick_create(device={device}) -> {rc}: {(msg or b'').decode()}")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rp_pick_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RpError(f"{what} -> {rc}: {(self._lib.rp_pick_last_error(self._h) or b'').decode()}")

    def set_reference(self, ref_xy, ref_pos=None, ref_theta=None, ref_curv=None, ref_curv_d=None, d_limit: Optional[float] = None):
        """The arguments of ``TrajectoryLifter.set_reference``: the tables of ``rp_build_reference`` -- vertices [n, 2], arc lengths,
        unwrapped orientations, curvature and its derivative, [n] each -- or the package's ``CoordinateSystem`` alone (its
        projection-domain limit unless ``d_limit`` is given).  Replaces the earlier table."""
        if ref_pos is None and hasattr(ref_xy, "ref_pos"):
            co = ref_xy
            ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d = co.reference, co.ref_pos, co.ref_theta, co.ref_curv, co.ref_curv_d
            if d_limit is None:
                d_limit = co.proj_domain_d_limit
        if ref_pos is None or ref_theta is None or ref_curv is None or ref_curv_d is None:
            raise ValueError("set_reference: ref_xy, ref_pos, ref_theta, ref_curv and ref_curv_d, or a CoordinateSystem")
        ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d = f64(ref_xy), f64(ref_pos), f64(ref_theta), f64(ref_curv), f64(ref_curv_d)
        n = ref_pos.shape[0]
        if ref_xy.shape != (n, 2) or any(q.shape != (n,) for q in (ref_pos, ref_theta, ref_curv, ref_curv_d)):
            raise ValueError(f"set_reference: shapes {ref_xy.shape}, {ref_pos.shape}, {ref_theta.shape}, {ref_curv.shape}, {ref_curv_d.shape}, "
                             f"not [n, 2] and four times [n]")
        self._check(self._lib.rp_pick_set_reference(self._h, n, dptr(ref_xy), dptr(ref_pos), dptr(ref_theta), dptr(ref_curv), dptr(ref_curv_d),
                                                    20.0 if d_limit is None else float(d_limit)), "rp_pick_set_reference")

    def set_obstacles(self, tables=None):
        """The tables ``RpContext.set_obstacles`` takes (``ObstacleTables``; None: empty); they replace the earlier ones."""
        from .collision import ObstacleTables
        tb = tables if tables is not None else ObstacleTables()
        nd, ns = tb.dyn_obb.shape[0], tb.dyn_obb.shape[1]
        self._check(self._lib.rp_pick_set_obstacles(
            self._h, len(tb.static_obb), dptr(tb.static_obb), len(tb.static_tri), dptr(tb.static_tri),
            len(tb.static_circ), dptr(tb.static_circ), nd, ns, int(tb.dyn_t0), dptr(tb.dyn_obb)), "rp_pick_set_obstacles")

    def pick(self, params: RpParams, cost: RpCost, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=None, theta0=None, poses: bool = True,
             swept: bool = False, want_planes: bool = False, want_hits: bool = False) -> TrajectoryPickResult:
        """The six planes: [K, n] (one trajectory may come as 1-D); ``lengths``: [K] valid poses per trajectory (None: n); ``theta0``:
        [K] orientations the trajectories start with (None: ``params.x0_orientation``).  ``poses``: the per-pose collision test at time
        index ``time_step0 + i * factor``; ``swept``: the continuous test of segment i at ``time_step0 + i``; neither: no collision test.
        ``want_planes``: the eight pose planes come back (otherwise none of them leaves the device); ``want_hits``: the first-hit arrays
        of the requested tests come back.  ``params``, ``cost``: what ``_capi.make_params`` and ``_capi.make_cost`` return."""
        s = np.atleast_2d(f64(s)) if np.ndim(s) != 2 else f64(s)
        K, n = s.shape
        s_dot, s_ddot = _plane(s_dot, (K, n), "s_dot"), _plane(s_ddot, (K, n), "s_ddot")
        d, d_dot, d_ddot = _plane(d, (K, n), "d"), _plane(d_dot, (K, n), "d_dot"), _plane(d_ddot, (K, n), "d_ddot")
        lens = None
        if lengths is not None:
            lens = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
            if lens.shape[0] != K:
                raise ValueError(f"pick: {lens.shape[0]} lengths for {K} trajectories")
        th0 = None
        if theta0 is not None:
            th0 = f64(theta0).reshape(-1)
            if th0.shape[0] != K:
                raise ValueError(f"pick: {th0.shape[0]} orientations for {K} trajectories")
        mode = (TRAJ_POSES if poses else 0) | (TRAJ_SWEPT if swept else 0)
        planes = [np.empty((K, n)) if want_planes else None for _ in PLANES]
        status, costs = np.empty(K, dtype=np.uint32), np.empty(K)
        first_pose = np.empty(K, dtype=np.int32) if want_hits and poses else None
        first_seg = np.empty(K, dtype=np.int32) if want_hits and swept else None
        res = RpPickResult()
        block = np.empty((RP_N_ARRAYS, n))
        as_ip = lambda a: a.ctypes.data_as(_ip) if a is not None else None   # noqa: E731
        self._check(self._lib.rp_pick_select(
            self._h, C.byref(params), C.byref(cost), mode, K, n, dptr(s), dptr(s_dot), dptr(s_ddot), dptr(d), dptr(d_dot), dptr(d_ddot),
            as_ip(lens), dptr(th0), 0, *[dptr(q) for q in planes], status.ctypes.data_as(_up), dptr(costs), as_ip(first_pose), as_ip(first_seg),
            C.byref(res), dptr(block)), "rp_pick_select")
        return TrajectoryPickResult(status, costs, int(res.best), float(res.best_cost), block if res.best >= 0 else None, int(res.n_feasible),
                                    int(res.n_collision), int(res.n_collision_before_best), np.array(res.reason_counts[:], dtype=np.int64),
                                    *planes, first_pose, first_seg)
