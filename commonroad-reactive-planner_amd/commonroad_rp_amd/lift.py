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
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpParams, dptr, f64
from ._session import as_ip

__all__ = ["TrajectoryLifter", "TrajectoryLiftResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_lift.so")
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


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_lift.so`` and declare every entry point of ``include/rp_lift.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


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


class TrajectoryLifter(_session.Session):
    """Owner of one ``rp_lift`` (one HIP stream, the segment table of one reference path, input and result buffers)."""

    _prefix, _load = "rp_lift", staticmethod(load_library)

    def set_reference(self, ref_xy, ref_pos=None, ref_theta=None, ref_curv=None, ref_curv_d=None, d_limit: Optional[float] = None):
        """The tables of ``rp_build_reference``: vertices [n, 2], arc lengths, unwrapped orientations, curvature and its derivative,
        [n] each; or the package's ``CoordinateSystem`` alone (its projection-domain limit unless ``d_limit`` is given).  Replaces the
        earlier table."""
        self._set_reference(ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, d_limit)

    def points(self, s, d, want_outside: bool = False):
        """(x, y, segment) of a batch of curvilinear points, in the shape of ``s``: NaN, NaN, -1 off the path.  With ``want_outside``
        the number of points off the path, counted on the device, comes fourth."""
        s, d = f64(s), f64(d)
        if s.shape != d.shape:
            raise ValueError(f"points: s of shape {s.shape}, d of shape {d.shape}")
        x, y, seg = np.empty(s.shape), np.empty(s.shape), np.empty(s.shape, dtype=np.int32)
        n_out = C.c_int64(0)
        self._call("points", s.size, dptr(s), dptr(d), dptr(x), dptr(y), as_ip(seg), C.byref(n_out))
        return (x, y, seg, int(n_out.value)) if want_outside else (x, y, seg)

    def lift(self, params: RpParams, s, s_dot, s_ddot, d, d_dot, d_ddot, lengths=None, theta0=None) -> TrajectoryLiftResult:
        """The six planes: [K, n] (one trajectory may come as 1-D); ``lengths``: [K] valid poses per trajectory (None: n); ``theta0``:
        [K] orientations the trajectories start with, read where one stands still from its first pose (None: ``params.x0_orientation``).
        ``params``: what ``_capi.make_params`` returns (dt, low_vel_mode, constraint_mask, x0_orientation and the vehicle limits are
        read)."""
        s, s_dot, s_ddot, d, d_dot, d_ddot = _session.six_planes("lift", s, s_dot, s_ddot, d, d_dot, d_ddot)
        K, n = s.shape
        lens, th0 = _session.lengths_of("lift", lengths, K), _session.theta0_of("lift", theta0, K)
        out = [np.empty((K, n)) for _ in range(8)]
        status = np.empty(K, dtype=np.uint32)
        counts = np.zeros(8, dtype=np.int64)
        first, n_feasible = C.c_int64(-1), C.c_int64(0)
        self._call("evaluate", C.byref(params), K, n, dptr(s), dptr(s_dot), dptr(s_ddot), dptr(d), dptr(d_dot), dptr(d_ddot), as_ip(lens), dptr(th0), 0,
                   *[dptr(q) for q in out], status.ctypes.data_as(_up), C.byref(first), C.byref(n_feasible), counts.ctypes.data_as(_lp))
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
