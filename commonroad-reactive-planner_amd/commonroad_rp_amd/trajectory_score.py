"""Curvilinear state, feasibility and cost of trajectories the caller brings: ctypes binding of ``include/rp_score.h``
(``librp_score.so``, built from ``csrc/rp_score.hip``).

The checkers and the clearance query cover the collision third of what the planner does with a candidate; ``TrajectoryScorer``
covers the other two thirds for K given trajectories of Cartesian poses -- their projection onto a reference path (s, d, theta_cl),
the reference planner's kinematic verdict (``_check_constraints``), its default cost, and the cheapest feasible one -- in one device
round trip.  ``project`` is the bare batch form of ``CoordinateSystem.convert_to_curvilinear_coords``.  A ``TrajectoryScorer``
shares nothing with an ``RpContext`` or the checkers.  There is NO CPU fallback: without the library creating one raises
``RpLibraryMissing``, without a GPU ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpCost, RpParams, dptr, f64
from ._session import as_ip

__all__ = ["TrajectoryScorer", "TrajectoryScoreResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_score.so")
ABI_VERSION = 1
MAX_POSES = 1 << 24
EXHAUSTIVE = 1   # RP_SCORE_EXHAUSTIVE: walk every segment, no pruning (a diagnostic; results do not depend on it)
RP_X, RP_Y, RP_THETA, RP_V, RP_A, RP_KAPPA, RP_N_ARRAYS = 0, 1, 2, 3, 4, 5, 14   # rows of a state block (include/rp_amd.h)

_dp, _ip, _up, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
_SIGNATURES = {
    "rp_score_abi_version": (C.c_int, []),
    "rp_score_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_score_destroy": (None, [C.c_void_p]),
    "rp_score_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_score_set_reference": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, _dp, C.c_double]),
    "rp_score_project": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _ip, _lp]),
    "rp_score_evaluate": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.POINTER(RpCost), C.c_int64, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _ip,
                                    C.c_uint32, _dp, _dp, _dp, _up, _dp, _lp, _dp, _lp, _lp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_score.so`` and declare every entry point of ``include/rp_score.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


@dataclasses.dataclass
class TrajectoryScoreResult:
    """``status``: [K] uint32, label | reason << 4 | first bad step << 8 (``RP_STATUS_*`` of include/rp_amd.h; label 1 feasible, 2
    infeasible); ``cost``: [K] float64, NaN where infeasible; ``best``: the k of the lexicographic minimum of (cost, k) over the
    feasible trajectories or -1; ``best_cost``: its cost or NaN; ``n_feasible``; ``reason_counts``: [8] int64, trajectories per reason
    code (1 velocity, 2 acceleration, 3 kappa, 4 kappa_dot, 5 yaw rate, 6 out of the projection domain); ``s``, ``d``, ``theta_cl``: [K, n]
    float64 or None (NaN outside the projection domain and behind a trajectory's end)."""
    status: np.ndarray
    cost: np.ndarray
    best: int
    best_cost: float
    n_feasible: int
    reason_counts: np.ndarray
    s: Optional[np.ndarray] = None
    d: Optional[np.ndarray] = None
    theta_cl: Optional[np.ndarray] = None

    @property
    def label(self) -> np.ndarray:
        return self.status & 3

    @property
    def reason(self) -> np.ndarray:
        return (self.status >> 4) & 7

    @property
    def step(self) -> np.ndarray:
        return (self.status >> 8) & 0xFFF


class TrajectoryScorer(_session.Session):
    """Owner of one ``rp_score`` (one HIP stream, the segment table of one reference path, pose and result buffers)."""

    _prefix, _load = "rp_score", staticmethod(load_library)

    def set_reference(self, ref_xy, ref_pos=None, ref_theta=None, d_limit: Optional[float] = None):
        """The tables ``RpContext.set_reference`` takes: vertices [n, 2], arc lengths [n], unwrapped orientations [n]; or the
        package's ``CoordinateSystem`` alone (its projection-domain limit unless ``d_limit`` is given).  Replaces the earlier table."""
        if ref_pos is None and hasattr(ref_xy, "ref_pos"):
            co = ref_xy
            ref_xy, ref_pos, ref_theta = co.reference, co.ref_pos, co.ref_theta
            if d_limit is None:
                d_limit = co.proj_domain_d_limit
        if ref_pos is None or ref_theta is None:
            raise ValueError("set_reference: ref_xy, ref_pos and ref_theta, or a CoordinateSystem")
        ref_xy, ref_pos, ref_theta = f64(ref_xy), f64(ref_pos), f64(ref_theta)
        n = ref_pos.shape[0]
        if ref_xy.shape != (n, 2) or ref_pos.shape != (n,) or ref_theta.shape != (n,):
            raise ValueError(f"set_reference: shapes {ref_xy.shape}, {ref_pos.shape}, {ref_theta.shape}, not [n, 2], [n], [n]")
        self._call("set_reference", n, dptr(ref_xy), dptr(ref_pos), dptr(ref_theta), 20.0 if d_limit is None else float(d_limit))

    def project(self, x, y, want_outside: bool = False):
        """(s, d, segment) of a batch of points, in the shape of ``x``: NaN, NaN, -1 outside the projection domain.  With
        ``want_outside`` the number of points outside, counted on the device, comes fourth."""
        x, y = f64(x), f64(y)
        if x.shape != y.shape:
            raise ValueError(f"project: x of shape {x.shape}, y of shape {y.shape}")
        s, d, seg = np.empty(x.shape), np.empty(x.shape), np.empty(x.shape, dtype=np.int32)
        n_out = C.c_int64(0)
        self._call("project", x.size, dptr(x), dptr(y), dptr(s), dptr(d), as_ip(seg), C.byref(n_out))
        return (s, d, seg, int(n_out.value)) if want_outside else (s, d, seg)

    def score(self, params: RpParams, cost: RpCost, x, y, theta, v=None, a=None, kappa=None, lengths=None, want_states: bool = False,
              flags: int = 0) -> TrajectoryScoreResult:
        """``x``, ``y``, ``theta`` (and ``v``, ``a``, ``kappa`` where a check or a cost term reads them): [K, n] (one trajectory may
        come as 1-D); ``lengths``: [K] valid poses per trajectory (None: n).  ``params``: what ``_capi.make_params`` returns (dt,
        constraint_mask and the vehicle limits are read), ``cost``: what ``_capi.make_cost`` returns."""
        x = _session.plane(x, None, "score", "x", "x")
        K, n = x.shape
        y, theta, v, a, kappa = (_session.plane(q, (K, n), "score", name, "x") for q, name in ((y, "y"), (theta, "theta"), (v, "v"), (a, "a"), (kappa, "kappa")))
        lens = _session.lengths_of("score", lengths, K)
        s, d, tcl = (np.empty((K, n)), np.empty((K, n)), np.empty((K, n))) if want_states else (None, None, None)
        status, cst = np.empty(K, dtype=np.uint32), np.empty(K, dtype=np.float64)
        counts = np.zeros(8, dtype=np.int64)
        best, best_cost, n_feasible = C.c_int64(-1), C.c_double(float("nan")), C.c_int64(0)
        self._call("evaluate", C.byref(params), C.byref(cost), K, n, dptr(x), dptr(y), dptr(theta), dptr(v), dptr(a), dptr(kappa), as_ip(lens), int(flags),
                   dptr(s), dptr(d), dptr(tcl), status.ctypes.data_as(_up), dptr(cst), C.byref(best), C.byref(best_cost), C.byref(n_feasible),
                   counts.ctypes.data_as(_lp))
        return TrajectoryScoreResult(status, cst, int(best.value), float(best_cost.value), int(n_feasible.value), counts, s, d, tcl)

    def score_states(self, params: RpParams, cost: RpCost, states, lengths=None, **kw) -> TrajectoryScoreResult:
        """``states``: the [C, RP_N_ARRAYS, N + 1] blocks of ``RpContext.fetch_states()``; rows ``RP_X``, ``RP_Y``, ``RP_THETA``,
        ``RP_V``, ``RP_A``, ``RP_KAPPA`` are read.  Everything else as ``score``."""
        states = np.asarray(states, dtype=np.float64)
        if states.ndim != 3 or states.shape[1] != RP_N_ARRAYS:
            raise ValueError(f"score_states: states of shape {states.shape}, not [C, RP_N_ARRAYS, N + 1]")
        return self.score(params, cost, states[:, RP_X, :], states[:, RP_Y, :], states[:, RP_THETA, :], v=states[:, RP_V, :], a=states[:, RP_A, :],
                          kappa=states[:, RP_KAPPA, :], lengths=lengths, **kw)
