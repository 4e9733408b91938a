"""Distance of trajectories the caller brings to the obstacles: ctypes binding of ``include/rp_clearance.h``
(``librp_clearance.so``, built from ``csrc/rp_clearance.hip``).

The checkers answer whether a pose collides; ``ClearanceQuery`` answers how close the poses of K given trajectories come to the
obstacles -- per pose, per trajectory (minimum, the pose and the obstacle that attain it) and as three scalars of the batch -- in
one device round trip: an obstacle-distance term of a plug-in ``CostFunction`` for a whole level (``query_states``), a safety
margin, a clearance profile.  A clearance of exactly 0.0 is the verdict of ``TrajectoryChecker``'s per-pose test.  A
``ClearanceQuery`` shares nothing with an ``RpContext`` or a checker.  There is NO CPU fallback: without the library creating one
raises ``RpLibraryMissing``, without a GPU ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpParams, dptr
from ._session import as_ip

__all__ = ["ClearanceQuery", "ClearanceResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_clearance.so")
ABI_VERSION = 1
MAX_POSES = 1 << 24
RP_X, RP_Y, RP_THETA, RP_N_ARRAYS = 0, 1, 2, 14   # rows of a state block (include/rp_amd.h)
TINY = 2.2250738585072014e-308   # RP_CLEARANCE_TINY: what a pair without a hit reports when its computed distance is not positive

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_SIGNATURES = {
    "rp_clearance_abi_version": (C.c_int, []),
    "rp_clearance_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_clearance_destroy": (None, [C.c_void_p]),
    "rp_clearance_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_clearance_set_obstacles": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "rp_clearance_query": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.c_int64, C.c_int32, _dp, _dp, _dp, _ip, C.c_double, C.c_double,
                                     _dp, _dp, _ip, _ip, _lp, _lp, _lp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_clearance.so`` and declare every entry point of ``include/rp_clearance.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


@dataclasses.dataclass
class ClearanceResult:
    """``pose_clearance``: [K, n] float64 or None (+inf above the cutoff, without an obstacle and behind a trajectory's end);
    ``min_clearance``: [K] float64; ``min_pose``: [K] int32, the smallest pose that attains it or -1; ``nearest``: [K] int32, the
    smallest obstacle id that attains it at that pose or -1 (ids: static rectangles, triangles, circles, then dynamic obstacles);
    ``first_clear``: smallest k with ``min_clearance[k] > margin`` or -1; ``n_below``: trajectories with ``min_clearance[k] <=
    margin``; ``best``: the k of the largest ``min_clearance`` (the smallest on ties), -1 for K == 0."""
    pose_clearance: Optional[np.ndarray]
    min_clearance: np.ndarray
    min_pose: np.ndarray
    nearest: np.ndarray
    first_clear: int
    n_below: int
    best: int


class ClearanceQuery(_session.Session):
    """Owner of one ``rp_clearance`` (one HIP stream, obstacle tables, pose and result buffers)."""

    _prefix, _load = "rp_clearance", staticmethod(load_library)

    def set_obstacles(self, tables=None):
        """The tables ``RpContext.set_obstacles`` takes (``ObstacleTables``; None: empty); they replace the earlier ones."""
        self._set_obstacles(tables)

    def query(self, params: RpParams, x, y, theta, lengths=None, cutoff: float = math.inf, margin: float = 0.0,
              want_pose_clearance: bool = False) -> ClearanceResult:
        """``x``, ``y``, ``theta``: [K, n] rear-axle poses (one trajectory may come as 1-D); ``lengths``: [K] valid poses per
        trajectory (None: n).  Pose i is measured against the static shapes and the dynamic obstacles at time index
        ``time_step0 + i * factor``.  ``cutoff``: clearances above it are reported as +inf (and cost little); ``margin``: what
        ``first_clear`` and ``n_below`` compare with.  ``params``: what ``_capi.make_params`` returns."""
        x, y, theta = _session.poses("query", x, y, theta)
        K, n = x.shape
        lens = _session.lengths_of("query", lengths, K)
        pose_clear = np.empty((K, n), dtype=np.float64) if want_pose_clearance else None
        min_clear = np.empty(K, dtype=np.float64)
        min_pose, nearest = np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
        first_clear, n_below, best = C.c_int64(-1), C.c_int64(0), C.c_int64(-1)
        self._call("query", C.byref(params), K, n, dptr(x), dptr(y), dptr(theta), as_ip(lens), float(cutoff), float(margin), dptr(pose_clear),
                   dptr(min_clear), as_ip(min_pose), as_ip(nearest), C.byref(first_clear), C.byref(n_below), C.byref(best))
        return ClearanceResult(pose_clear, min_clear, min_pose, nearest, int(first_clear.value), int(n_below.value), int(best.value))

    def query_states(self, params: RpParams, states, lengths=None, **kw) -> ClearanceResult:
        """``states``: the [C, RP_N_ARRAYS, N + 1] blocks of ``RpContext.fetch_states()``; rows ``RP_X``, ``RP_Y``, ``RP_THETA`` are
        the poses.  Everything else as ``query``: a plug-in cost gets its obstacle term for a whole level in one call."""
        states = np.asarray(states, dtype=np.float64)
        if states.ndim != 3 or states.shape[1] != RP_N_ARRAYS:
            raise ValueError(f"query_states: states of shape {states.shape}, not [C, RP_N_ARRAYS, N + 1]")
        return self.query(params, states[:, RP_X, :], states[:, RP_Y, :], states[:, RP_THETA, :], lengths=lengths, **kw)
