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
import os
import sys
from typing import Optional

import numpy as np

from ._capi import RpError, RpLibraryMissing, RpParams, dptr, f64

__all__ = ["TrajectoryChecker", "TrajectoryCheckResult", "load_library", "EXPORTED_SYMBOLS", "LIB_PATH"]

LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "librp_check.so")
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

_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load ``librp_check.so`` and declare every entry point of ``include/rp_check.h``."""
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
    if lib.rp_checker_abi_version() != ABI_VERSION:
        raise RpError(f"{path}: ABI version {lib.rp_checker_abi_version()}, this binding speaks {ABI_VERSION}")
    if path == LIB_PATH:
        _lib = lib
    return lib


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


class TrajectoryChecker:
    """Owner of one ``rp_checker`` (one HIP stream, obstacle tables, pose and result buffers)."""

    def __init__(self, device: int = 0, library: Optional[str] = None):
        self._lib = load_library(library)
        self._h = C.c_void_p()
        rc = self._lib.rp_checker_create(C.byref(self._h), int(device))
        if rc != 0:
            msg = self._lib.rp_checker_last_error(self._h) if self._h else b"rp_checker_create failed"
            self.close()
            raise RpError(f"rp_checker_create(device={device}) -> {rc}: {(msg or b'').decode()}")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rp_checker_destroy(self._h)
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
            raise RpError(f"{what} -> {rc}: {(self._lib.rp_checker_last_error(self._h) or b'').decode()}")

    def set_obstacles(self, tables=None):
        """The tables ``RpContext.set_obstacles`` takes (``ObstacleTables``; None: empty); they replace the earlier ones."""
        from .collision import ObstacleTables
        tb = tables if tables is not None else ObstacleTables()
        nd, ns = tb.dyn_obb.shape[0], tb.dyn_obb.shape[1]
        self._check(self._lib.rp_checker_set_obstacles(
            self._h, len(tb.static_obb), dptr(tb.static_obb), len(tb.static_tri), dptr(tb.static_tri),
            len(tb.static_circ), dptr(tb.static_circ), nd, ns, int(tb.dyn_t0), dptr(tb.dyn_obb)), "rp_checker_set_obstacles")

    def check(self, params: RpParams, x, y, theta, lengths=None, poses: bool = True, swept: bool = False,
              want_pose_hits: bool = False) -> TrajectoryCheckResult:
        """``x``, ``y``, ``theta``: [K, n] rear-axle poses (one trajectory may come as 1-D); ``lengths``: [K] valid poses per
        trajectory (None: n).  ``poses``: the per-pose test at time index ``time_step0 + i * factor``; ``swept``: the continuous
        test of segment i at ``time_step0 + i``.  ``params``: what ``_capi.make_params`` returns."""
        x, y, theta = (np.atleast_2d(f64(a)) if np.ndim(a) != 2 else f64(a) for a in (x, y, theta))
        if not (x.ndim == y.ndim == theta.ndim == 2 and x.shape == y.shape == theta.shape):
            raise ValueError(f"check: x, y, theta differ in shape ({x.shape}, {y.shape}, {theta.shape}) or are not [K, n]")
        K, n = x.shape
        lens = None
        if lengths is not None:
            lens = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
            if lens.shape[0] != K:
                raise ValueError(f"check: {lens.shape[0]} lengths for {K} trajectories")
        mode = (TRAJ_POSES if poses else 0) | (TRAJ_SWEPT if swept else 0)
        first_pose = np.empty(K, dtype=np.int32) if poses else None
        first_seg = np.empty(K, dtype=np.int32) if swept else None
        hits = np.zeros((K, n), dtype=np.uint8) if want_pose_hits else None
        first_free, n_hit = C.c_int64(-1), C.c_int64(0)
        as_ip = lambda a: a.ctypes.data_as(_ip) if a is not None else None   # noqa: E731
        self._check(self._lib.rp_checker_check(
            self._h, C.byref(params), mode, K, n, dptr(x), dptr(y), dptr(theta), as_ip(lens), as_ip(first_pose), as_ip(first_seg),
            hits.ctypes.data_as(C.POINTER(C.c_uint8)) if hits is not None else None, C.byref(first_free), C.byref(n_hit)),
            "rp_checker_check")
        return TrajectoryCheckResult(first_pose, first_seg, hits.astype(bool) if hits is not None else None,
                                     int(first_free.value), int(n_hit.value))
