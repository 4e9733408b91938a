"""Batch collision check of trajectories the caller brings: ctypes binding of ``include/rp_check.h``
(``librp_check.so``, built from ``csrc/rp_check.hip``).

The planner's own calls answer which candidate of ITS sampling grid is free; ``TrajectoryChecker`` answers it for K given
trajectories in one device round trip -- the K cheapest candidates of a level, motion-primitive sets, fail-safe manoeuvres,
prediction ensembles -- with both tests of ``ReactivePlanner._check_collisions`` (reactive_planner.py:1033-1058).  A checker
shares nothing with an ``RpContext``; both can live side by side.  There is NO CPU fallback: without the library creating a
checker raises ``RpLibraryMissing``, without a GPU ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpParams, dptr
from ._session import as_ip

__all__ = ["TrajectoryChecker", "TrajectoryCheckResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_check.so")
ABI_VERSION = 1
TRAJ_POSES, TRAJ_SWEPT = 1, 2
MAX_POSES = 1 << 24

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
_SIGNATURES = {
    "rp_checker_abi_version": (C.c_int, []),
    "rp_checker_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_checker_destroy": (None, [C.c_void_p]),
    "rp_checker_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_checker_set_obstacles": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "rp_checker_check": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.c_uint32, C.c_int64, C.c_int32, _dp, _dp, _dp, _ip, _ip, _ip,
                                   C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_check.so`` and declare every entry point of ``include/rp_check.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


@dataclasses.dataclass
class TrajectoryCheckResult:
    """``first_pose_hit`` / ``first_segment_hit``: [K] int32, smallest colliding pose / segment of each trajectory or -1 (None when
    the test was not asked for); ``pose_hits``: [K, n] bool or None; ``first_free``: smallest k without any requested hit, -1 if
    none; ``n_hit``: trajectories with a hit."""
    first_pose_hit: Optional[np.ndarray]
    first_segment_hit: Optional[np.ndarray]
    pose_hits: Optional[np.ndarray]
    first_free: int
    n_hit: int


class TrajectoryChecker(_session.Session):
    """Owner of one ``rp_checker`` (one HIP stream, obstacle tables, pose and result buffers)."""

    _prefix, _load = "rp_checker", staticmethod(load_library)

    def set_obstacles(self, tables=None):
        """The tables ``RpContext.set_obstacles`` takes (``ObstacleTables``; None: empty); they replace the earlier ones."""
        self._set_obstacles(tables)

    def check(self, params: RpParams, x, y, theta, lengths=None, poses: bool = True, swept: bool = False,
              want_pose_hits: bool = False) -> TrajectoryCheckResult:
        """``x``, ``y``, ``theta``: [K, n] rear-axle poses (one trajectory may come as 1-D); ``lengths``: [K] valid poses per
        trajectory (None: n).  ``poses``: the per-pose test at time index ``time_step0 + i * factor``; ``swept``: the continuous
        test of segment i at ``time_step0 + i``.  ``params``: what ``_capi.make_params`` returns."""
        x, y, theta = _session.poses("check", x, y, theta)
        K, n = x.shape
        lens = _session.lengths_of("check", lengths, K)
        mode = (TRAJ_POSES if poses else 0) | (TRAJ_SWEPT if swept else 0)
        first_pose = np.empty(K, dtype=np.int32) if poses else None
        first_seg = np.empty(K, dtype=np.int32) if swept else None
        hits = np.zeros((K, n), dtype=np.uint8) if want_pose_hits else None
        first_free, n_hit = C.c_int64(-1), C.c_int64(0)
        self._call("check", C.byref(params), mode, K, n, dptr(x), dptr(y), dptr(theta), as_ip(lens), as_ip(first_pose), as_ip(first_seg),
                   hits.ctypes.data_as(C.POINTER(C.c_uint8)) if hits is not None else None, C.byref(first_free), C.byref(n_hit))
        return TrajectoryCheckResult(first_pose, first_seg, hits.astype(bool) if hits is not None else None,
                                     int(first_free.value), int(n_hit.value))
