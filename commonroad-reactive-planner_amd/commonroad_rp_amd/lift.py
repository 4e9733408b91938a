"""Cartesian states and kinematic verdict of curvilinear trajectories the caller brings: ctypes binding of ``include/rp_lift.h``
(``librp_lift.so``, built from ``csrc/rp_lift.hip``).

``TrajectoryScorer`` maps given Cartesian trajectories into the frame of a reference path; ``TrajectoryLifter`` is the opposite
direction for K given trajectories s, s', s'', d, d', d'' -- no polynomial pair is assumed: x, y, theta, v, a, kappa, kappa_dot and
theta_cl as ``ReactivePlanner._check_kinematics`` computes them in draw mode, with its verdict, in one device round trip.
``lift_states`` returns the blocks ``TrajectoryChecker``, ``ClearanceQuery.query_states`` and ``TrajectoryScorer.score_states`` take.
``points`` is the bare batch form of ``CoordinateSystem.convert_to_cartesian_coords``.  A ``TrajectoryLifter`` shares nothing with an
``RpContext``, the checkers or the scorer.  There is NO CPU fallback: without the library creating one raises ``RpLibraryMissing``,
without a GPU ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import sys
from typing import Optional

import numpy as np

from ._capi import RpError, RpLibraryMissing, RpParams, dptr, f64

__all__ = ["TrajectoryLifter", "TrajectoryLiftResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "librp_lift.so")
ABI_VERSION = 1
MAX_POSES = 1 << 24
# rows of a state block (include/rp_amd.h)
RP_X, RP_Y, RP_THETA, RP_V, RP_A, RP_KAPPA, RP_KAPPA_DOT, RP_S, RP_D, RP_THETA_CL, RP_S_DOT, RP_S_DDOT, RP_D_DOT, RP_D_DDOT, RP_N_ARRAYS = range(15)

_dp, _ip, _up, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
_SIGNATURES = {
    "rp_lift_abi_version": (C.c_int, []),
    "rp_lift_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_lift_destroy": (None, [C.c_void_p]),
    "rp_lift_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_lift_set_reference": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_double]),
    "rp_lift_points": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _ip, _lp]),
    "rp_lift_evaluate": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.c_int64, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp, C.c_uint32,
                                   _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _up, _lp, _lp, _lp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_lift.so`` and declare every entry point of ``include/rp_lift.h``."""
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
    if lib.rp_lift_abi_version() != ABI_VERSION:
        raise RpError(f"{path}: ABI version {lib.rp_lift_abi_version()}, this binding speaks {ABI_VERSION}")
    if path == LIB_PATH:
        _lib = lib
    return lib


@dataclasses.dataclass
class TrajectoryLiftResult:
    """``status``: [K] uint32, label | reason << 4 | first bad step << 8 (``RP_STATUS_*`` of include/rp_amd.h; label 1 feasible, 2
    infeasible); ``first_feasible``: the smallest feasible k or -1; ``n_feasible``; ``reason_counts``: [8] int64, trajectories per reason
    code (1 velocity, 2 acceleration, 3 kappa, 4 kappa_dot, 5 yaw rate, 6 off the path); ``x`` .. ``theta_cl``: [K, n] float64 (NaN from
    the pose that leaves the path and behind a trajectory's end; ``x``, ``y`` also where |d| is beyond the limit)."""
    status: np.ndarray
    first_feasible: int
    n_feasible: int
    reason_counts: np.ndarray
    x: np.ndarray
    y: np.ndarray
    theta: np.ndarray
    v: np.ndarray
    a: np.ndarray
    kappa: np.ndarray
    kappa_dot: np.ndarray
    theta_cl: np.ndarray

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
        raise ValueError(f"lift: {name} of shape {a.shape}, s of shape {shape}")
    return a


class TrajectoryLifter:
    """Owner of one ``rp_lift`` (one HIP stream, the segment table of one reference path, input and result buffers)."""

    def __init__(self, device: int = 0, library: Optional[str] = None):
        self._lib = load_library(library)
        self._h = C.c_void_p()
        rc = self._lib.rp_lift_create(C.byref(self._h), int(device))
        if rc != 0:
            msg = self._lib.rp_lift_last_error(self._h) if self._h else b"rp_lift_create failed"
            self.close()
            raise RpError(f"rp_lift_create(device={device}) -> {rc}: {(msg or b'').decode()}")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rp_lift_destroy(self._h)
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
            raise RpError(f"{what} -> {rc}: {(self._lib.rp_lift_last_error(self._h) or b'').decode()}")

    def set_reference(self, ref_xy, ref_pos=None, ref_theta=None, ref_curv=None, ref_curv_d=None, d_limit: Optional[float] = None):
        """The tables of ``rp_build_reference``: vertices [n, 2], arc lengths, unwrapped orientations, curvature and its derivative,
        [n] each; or the package's ``CoordinateSystem`` alone (its projection-domain limit unless ``d_limit`` is given).  Replaces the
        earlier table."""
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
        self._check(self._lib.rp_lift_set_reference(self._h, n, dptr(ref_xy), dptr(ref_pos), dptr(ref_theta), dptr(ref_curv), dptr(ref_curv_d),
                                                    20.0 if d_limit is None else float(d_limit)), "rp_lift_set_reference")

    def points(self, s, d, want_outside: bool = False):
        """(x, y, segment) of a batch of curvilinear points, in the shape of ``s``: NaN, NaN, -1 off the path.  With ``want_outside``
        the number of points off the path, counted on the device, comes fourth."""
        s, d = f64(s), f64(d)
        if s.shape != d.shape:
            raise ValueError(f"points: s of shape {s.shape}, d of shape {d.shape}")
        x, y, seg = np.empty(s.shape), np.empty(s.shape), np.empty(s.shape, dtype=np.int32)
        n_out = C.c_int64(0)
        self._check(self._lib.rp_lift_points(self._h, s.size, dptr(s), dptr(d), dptr(x), dptr(y), seg.ctypes.data_as(_ip), C.byref(n_out)),
                    "rp_lift_points")
        return (x, y, seg, int(n_out.value)) if want_outside else (x, y, seg)

    def lift(self, params: RpParams, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=None, theta0=None) -> TrajectoryLiftResult:
        """The six planes: [K, n] (one trajectory may come as 1-D); ``lengths``: [K] valid poses per trajectory (None: n); ``theta0``:
        [K] orientations the trajectories start with, read where one stands still from its first pose (None: ``params.x0_orientation``).
        ``params``: what ``_capi.make_params`` returns (dt, low_vel_mode, constraint_mask, x0_orientation and the vehicle limits are
        read)."""
        s = np.atleast_2d(f64(s)) if np.ndim(s) != 2 else f64(s)
        K, n = s.shape
        s_dot, s_ddot = _plane(s_dot, (K, n), "s_dot"), _plane(s_ddot, (K, n), "s_ddot")
        d, d_dot, d_ddot = _plane(d, (K, n), "d"), _plane(d_dot, (K, n), "d_dot"), _plane(d_ddot, (K, n), "d_ddot")
        lens = None
        if lengths is not None:
            lens = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
            if lens.shape[0] != K:
                raise ValueError(f"lift: {lens.shape[0]} lengths for {K} trajectories")
        th0 = None
        if theta0 is not None:
            th0 = f64(theta0).reshape(-1)
            if th0.shape[0] != K:
                raise ValueError(f"lift: {th0.shape[0]} orientations for {K} trajectories")
        out = [np.empty((K, n)) for _ in range(8)]
        status = np.empty(K, dtype=np.uint32)
        counts = np.zeros(8, dtype=np.int64)
        first, n_feasible = C.c_int64(-1), C.c_int64(0)
        self._check(self._lib.rp_lift_evaluate(
            self._h, C.byref(params), K, n, dptr(s), dptr(s_dot), dptr(s_ddot), dptr(d), dptr(d_dot), dptr(d_ddot),
            lens.ctypes.data_as(_ip) if lens is not None else None, dptr(th0), 0, *[dptr(q) for q in out], status.ctypes.data_as(_up),
            C.byref(first), C.byref(n_feasible), counts.ctypes.data_as(_lp)), "rp_lift_evaluate")
        return TrajectoryLiftResult(status, int(first.value), int(n_feasible.value), counts, *out)

    def lift_states(self, params: RpParams, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=None, theta0=None) -> np.ndarray:
        """The same arguments as ``lift``; returns the [K, RP_N_ARRAYS, n] blocks in the row layout of ``RpContext.fetch_states()``:
        rows x, y, theta, v, a, kappa, kappa_dot and theta_cl from the device, rows s, d and their four derivatives the inputs."""
        r = self.lift(params, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=lengths, theta0=theta0)
        K, n = r.x.shape
        states = np.empty((K, RP_N_ARRAYS, n))
        for row, q in ((RP_X, r.x), (RP_Y, r.y), (RP_THETA, r.theta), (RP_V, r.v), (RP_A, r.a), (RP_KAPPA, r.kappa), (RP_KAPPA_DOT, r.kappa_dot),
                       (RP_THETA_CL, r.theta_cl), (RP_S, s), (RP_S_DOT, s_dot), (RP_S_DDOT, s_ddot), (RP_D, d), (RP_D_DOT, d_dot), (RP_D_DDOT, d_ddot)):
            states[:, row, :] = np.asarray(q, dtype=np.float64).reshape(K, n)
        return states
