"""Collision check of given trajectories against an ensemble of predictions: ctypes binding of ``include/rp_ensemble.h``
(``librp_ensemble.so``, built from ``csrc/rp_ensemble.hip``).

``TrajectoryChecker`` answers which of K given trajectories is free against ONE dynamic-obstacle table.  ``EnsembleChecker``
holds M tables -- M sampled futures of the same obstacles, the "members" -- and answers in one device round trip, per
trajectory, in how many members it collides, where first in each, and which is the first trajectory that collides in at most
``max_members_hit`` of them.  The tests are those of ``TrajectoryChecker`` (both tests of ``ReactivePlanner._check_collisions``,
reactive_planner.py:1033-1058).  An ensemble checker shares nothing with an ``RpContext`` or a ``TrajectoryChecker``; all can
live side by side.  There is NO CPU fallback: without the library creating one raises ``RpLibraryMissing``, without a GPU
``RpError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _session
from ._capi import RpParams, dptr
from ._session import as_ip

__all__ = ["EnsembleChecker", "EnsembleCheckResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = _session.lib_path("librp_ensemble.so")
ABI_VERSION = 1
TRAJ_POSES, TRAJ_SWEPT = 1, 2
MAX_MEMBERS = 4096
MAX_DYN_ROWS = 1 << 22
MAX_POSES = 1 << 24
MAX_VERDICTS = 1 << 24

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_SIGNATURES = {
    "rp_ensemble_abi_version": (C.c_int, []),
    "rp_ensemble_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "rp_ensemble_destroy": (None, [C.c_void_p]),
    "rp_ensemble_last_error": (C.c_char_p, [C.c_void_p]),
    "rp_ensemble_set_static": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp]),
    "rp_ensemble_set_members": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "rp_ensemble_check": (C.c_int, [C.c_void_p, C.POINTER(RpParams), C.c_uint32, C.c_int64, C.c_int32, _dp, _dp, _dp, _ip, C.c_int32,
                                    _ip, _ip, _ip, _lp, _lp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_ensemble.so`` and declare every entry point of ``include/rp_ensemble.h``."""
    return _session.load_library(path, LIB_PATH, _SIGNATURES, ABI_VERSION)


@dataclasses.dataclass
class EnsembleCheckResult:
    """``first_pose_hit`` / ``first_segment_hit``: [K, M] int32, smallest colliding pose / segment of each trajectory in each member
    or -1 (None when the test was not asked for); ``members_hit``: [K] int32, members in which the trajectory has any requested hit;
    ``first_free``: smallest k with ``members_hit[k] <= max_members_hit``, -1 if none; ``n_over``: trajectories above it."""
    first_pose_hit: Optional[np.ndarray]
    first_segment_hit: Optional[np.ndarray]
    members_hit: np.ndarray
    first_free: int
    n_over: int


class EnsembleChecker(_session.Session):
    """Owner of one ``rp_ensemble`` (one HIP stream, static shapes, member tables, pose and result buffers)."""

    _prefix, _load = "rp_ensemble", staticmethod(load_library)

    def __init__(self, device: int = 0, library: Optional[str] = None):
        super().__init__(device, library)
        self.n_members = 1

    def set_static(self, tables=None):
        """The static shapes of an ``ObstacleTables`` (None: none); they replace the earlier ones, the members stay."""
        self._set_static(tables)

    def set_members(self, members, dyn_t0: int = 0):
        """``members``: [M, n_dyn, n_steps, 5] dynamic rectangles (rows of ``ObstacleTables.dyn_obb``, cx = NaN: absent) for
        scenario time steps ``dyn_t0 ..``; they replace the earlier members, the static shapes stay; a call that fails leaves the
        earlier members."""
        mem, M, nd, ns = _session.members_args(members)
        self._call("set_members", M, nd, ns, int(dyn_t0), dptr(mem) if mem.size else None)
        self.n_members = M

    def set_obstacles(self, tables=None, members=None, dyn_t0: Optional[int] = None):
        """Static shapes from ``tables`` (``ObstacleTables``; None: none).  ``members``: [M, n_dyn, n_steps, 5] with ``dyn_t0``
        (None: ``tables.dyn_t0``); ``members`` None: one member from ``tables.dyn_obb`` and ``tables.dyn_t0``."""
        from .collision import ObstacleTables
        tb = tables if tables is not None else ObstacleTables()
        self.set_static(tb)
        if members is None:
            self.set_members(tb.dyn_obb[None], tb.dyn_t0 if dyn_t0 is None else dyn_t0)
        else:
            self.set_members(members, tb.dyn_t0 if dyn_t0 is None else dyn_t0)

    def check(self, params: RpParams, x, y, theta, lengths=None, poses: bool = True, swept: bool = False,
              max_members_hit: int = 0) -> EnsembleCheckResult:
        """``x``, ``y``, ``theta``: [K, n] rear-axle poses (one trajectory may come as 1-D); ``lengths``: [K] valid poses per
        trajectory (None: n).  ``poses``: the per-pose test at time index ``time_step0 + i * factor``; ``swept``: the continuous
        test of segment i at ``time_step0 + i``.  ``params``: what ``_capi.make_params`` returns."""
        x, y, theta = _session.poses("check", x, y, theta)
        K, n = x.shape
        M = self.n_members
        lens = _session.lengths_of("check", lengths, K)
        mode = (TRAJ_POSES if poses else 0) | (TRAJ_SWEPT if swept else 0)
        first_pose = np.empty((K, M), dtype=np.int32) if poses else None
        first_seg = np.empty((K, M), dtype=np.int32) if swept else None
        members_hit = np.zeros(K, dtype=np.int32)
        first_free, n_over = C.c_int64(-1), C.c_int64(0)
        self._call("check", C.byref(params), mode, K, n, dptr(x), dptr(y), dptr(theta), as_ip(lens), int(max_members_hit), as_ip(first_pose),
                   as_ip(first_seg), as_ip(members_hit), C.byref(first_free), C.byref(n_over))
        return EnsembleCheckResult(first_pose, first_seg, members_hit, int(first_free.value), int(n_over.value))
