"""What the bindings of the trajectory libraries share: loading a library and declaring its entry points, the owner of one opaque
object, and the marshalling of the arguments they have in common.  It names no library: each module passes its path, its signatures,
its ABI version and the prefix of its C names.  There is NO CPU fallback here either: a missing library is ``RpLibraryMissing``, a
refused or failed call ``RpError``.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

import numpy as np

from ._capi import RpError, RpLibraryMissing, dptr, f64

_ip = C.POINTER(C.c_int32)
_default_libs = {}   # a module's LIB_PATH -> its library; a path given explicitly is loaded anew each time


def lib_path(name: str) -> str:
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", name)


def load_library(path: Optional[str], default: str, signatures: dict, abi_version: int) -> C.CDLL:
    """Load the library at ``path`` (None: ``default``, loaded once) and declare ``signatures``; its ``*_abi_version`` must answer
    ``abi_version``."""
    if path is None and default in _default_libs:
        return _default_libs[default]
    path = path or default
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
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    version = getattr(lib, next(name for name in signatures if name.endswith("_abi_version")))()
    if version != abi_version:
        raise RpError(f"{path}: ABI version {version}, this binding speaks {abi_version}")
    if path == default:
        _default_libs[default] = lib
    return lib


def as_ip(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def plane(a, shape, what: str, name: str, first: str):
    """``a`` as a [K, n] float64 plane (one trajectory may come as 1-D; None stays None); ``shape``: the first plane's, None for the
    first plane itself."""
    if a is None:
        return None
    a = np.atleast_2d(f64(a)) if np.ndim(a) != 2 else f64(a)
    if shape is not None and a.shape != shape:
        raise ValueError(f"{what}: {name} of shape {a.shape}, {first} of shape {shape}")
    return a


def poses(what: str, x, y, theta):
    """The three [K, n] pose planes of the checkers and the clearance query."""
    x, y, theta = (plane(a, None, what, "", "") for a in (x, y, theta))
    if not (x.ndim == y.ndim == theta.ndim == 2 and x.shape == y.shape == theta.shape):
        raise ValueError(f"{what}: x, y, theta differ in shape ({x.shape}, {y.shape}, {theta.shape}) or are not [K, n]")
    return x, y, theta


def six_planes(what: str, s, s_dot, s_ddot, d, d_dot, d_ddot):
    """The six [K, n] curvilinear planes of the lifter and the picks."""
    s = plane(s, None, what, "s", "s")
    rest = [plane(a, s.shape, what, name, "s") for a, name in ((s_dot, "s_dot"), (s_ddot, "s_ddot"), (d, "d"), (d_dot, "d_dot"), (d_ddot, "d_ddot"))]
    return [s] + rest


def lengths_of(what: str, lengths, K: int):
    """[K] int32 valid poses per trajectory, or None"""
    if lengths is None:
        return None
    lens = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
    if lens.shape[0] != K:
        raise ValueError(f"{what}: {lens.shape[0]} lengths for {K} trajectories")
    return lens


def theta0_of(what: str, theta0, K: int):
    """[K] float64 orientations the trajectories start with, or None"""
    if theta0 is None:
        return None
    th0 = f64(theta0).reshape(-1)
    if th0.shape[0] != K:
        raise ValueError(f"{what}: {th0.shape[0]} orientations for {K} trajectories")
    return th0


def static_args(tables):
    """(tables or empty ones, the six arguments every set call of static shapes takes)"""
    from .collision import ObstacleTables
    tb = tables if tables is not None else ObstacleTables()
    return tb, (len(tb.static_obb), dptr(tb.static_obb), len(tb.static_tri), dptr(tb.static_tri), len(tb.static_circ), dptr(tb.static_circ))


def members_args(members):
    """``members`` as [M, n_dyn, n_steps, 5] float64, and M, n_dyn, n_steps"""
    mem = f64(members)
    if mem.ndim != 4 or mem.shape[3] != 5:
        raise ValueError(f"set_members: members must be [M, n_dyn, n_steps, 5], got {mem.shape}")
    return (mem,) + tuple(mem.shape[:3])


class Session:
    """Owner of one opaque object of the library ``_load`` returns, behind the C names ``<_prefix>_create``, ``_destroy`` and
    ``_last_error``.  A subclass sets ``_prefix`` and ``_load``."""
    _prefix = ""
    _load = None

    def __init__(self, device: int = 0, library: Optional[str] = None):
        self._lib = type(self)._load(library)
        self._h = C.c_void_p()
        rc = self._fn("create")(C.byref(self._h), int(device))
        if rc != 0:
            msg = self._fn("last_error")(self._h) if self._h else f"{self._prefix}_create failed".encode()
            self.close()
            raise RpError(f"{self._prefix}_create(device={device}) -> {rc}: {(msg or b'').decode()}")
        self.device = device

    def _fn(self, name: str):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
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
            raise RpError(f"{what} -> {rc}: {(self._fn('last_error')(self._h) or b'').decode()}")

    def _call(self, name: str, *args):
        """``<_prefix>_<name>(handle, *args)``; anything but RP_OK raises with the library's message"""
        rc = self._fn(name)(self._h, *args)
        if rc != 0:
            self._check(rc, f"{self._prefix}_{name}")

    def _set_obstacles(self, tables):
        tb, static = static_args(tables)
        self._call("set_obstacles", *static, tb.dyn_obb.shape[0], tb.dyn_obb.shape[1], int(tb.dyn_t0), dptr(tb.dyn_obb))

    def _set_static(self, tables):
        self._call("set_static", *static_args(tables)[1])

    def _set_reference(self, ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, d_limit):
        """Tables or a ``CoordinateSystem`` alone -> ``<_prefix>_set_reference`` with curvature and its derivative"""
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
        self._call("set_reference", n, dptr(ref_xy), dptr(ref_pos), dptr(ref_theta), dptr(ref_curv), dptr(ref_curv_d),
                   20.0 if d_limit is None else float(d_limit))
