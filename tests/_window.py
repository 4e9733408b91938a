"""The reference-table window of the single-launch kernel (csrc/rp_table_window.h, the LON_FUSED prologue of csrc/rp_kernels.h), restated
in NumPy for tests/test_table_window_host.py and tests/test_table_window_gpu.py.

Three things live here:

  * the host rule and the bucket table AS THE LIBRARY BUILDS THEM, through lib/librp_windowtest.so (rule_window, bucket_table);
  * the set of table entries a lookup touches for a given s (lookup_reads) -- restated from the kernels, NOT taken from the rule, so
    that the two can be held against each other;
  * the prologue's item set (workgroup_items) and the class of every workgroup of a plan: does any of its items leave the window?

Where the restatement comes from (csrc/):
  rp_device.h   upper_bound_bucket          bucket index with its clamp, bucket[b], one backward and two forward fix-ups
  rp_kernels.h  lon_step_part               ub -> s_idx -> (k0, k1) with the wrap-around pair (n - 1, 0); foot point k, k + 1 clamped
                                            to [0, n - 2]; rows read at k0: pos, invlen, theta, curv, curv_d; at k1: theta, curv, curv_d;
                                            at k: pos, invlen, x, y, tx, ty; at k + 1: x, y, tx, ty
  rp_kernels.h  LON_FUSED prologue          candidates of workgroup b: slots [b * GPB, (b + 1) * GPB), GPB = 256 / lanes; its pairs
                                            p = candidate // nD; items (p, i) for i = 0 .. N, valid or extrapolated alike; an item is
                                            "inside" if win_s_lo <= s < win_s_hi
  rp_kernels.h  lon_pair_make               the longitudinal polynomial (rp_device.h: quartic_coeffs / quintic_coeffs), s = lon.pos(i dt)
"""
import collections
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "commonroad-reactive-planner_amd", "lib", "librp_windowtest.so")
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int32)
LON_VELOCITY_KEEPING, LON_STOPPING = 0, 1   # include/rp_amd.h
RP_BLOCK = 256                              # threads of a workgroup (rp_kernels.h)

Window = collections.namedtuple("Window", "k0 n shift b0 nb s_lo s_hi")   # n == 0: the whole block
Buckets = collections.namedtuple("Buckets", "table nb inv_h")             # nb == 0: no table (the kernels search)


def load():
    L = C.CDLL(LIB)
    L.rptw_test_buckets.argtypes = [DP, C.c_int, IP, C.c_int, DP]
    L.rptw_test_window.argtypes = [DP, C.c_int, C.c_int, C.c_double, C.c_int, DP, DP, C.c_int, DP, C.c_int, IP, DP]
    L.rptw_test_constant.argtypes = [C.c_int]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load()
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, (a.ctypes.data_as(DP) if a.size else None)


def bucket_table(pos) -> Buckets:
    """the bucket table rp_set_reference uploads for the arclengths `pos`"""
    pos, pp = _d(pos)
    inv_h = C.c_double(0.0)
    nb = lib().rptw_test_buckets(pp, len(pos), None, 0, C.byref(inv_h))
    tab = np.zeros(max(nb, 1), dtype=np.int32)
    lib().rptw_test_buckets(pp, len(pos), tab.ctypes.data_as(IP), nb, C.byref(inv_h))
    return Buckets(tab[:nb], nb, inv_h.value)


def rule_window(pos, bk: Buckets, lon_mode, x0_lon, T, L) -> Window:
    """the window rp_plan puts into the kernel arguments of a grid plan on this reference (option "table_window" = 1)"""
    pos, pp = _d(pos)
    x0, px = _d(x0_lon)
    T, pT = _d(T)
    L, pL = _d(L)
    wi = np.zeros(5, dtype=np.int32)
    ws = np.zeros(2)
    lib().rptw_test_window(pp, len(pos), bk.nb, bk.inv_h, int(lon_mode), px, pT, len(T), pL, len(L), wi.ctypes.data_as(IP), ws.ctypes.data_as(DP))
    return Window(int(wi[0]), int(wi[1]), int(wi[2]), int(wi[3]), int(wi[4]), float(ws[0]), float(ws[1]))


# ---- what a lookup touches ------------------------------------------------------------------------------------------------------
Reads = collections.namedtuple("Reads", "ub vmin vmax bucket")


def lookup_reads(pos, bk: Buckets, s) -> Reads:
    """For every s: the result of upper_bound_bucket, the smallest and the largest VERTEX index any row is read at (the bucket
    fix-ups, k0 / k1, k / k + 1), and the bucket entry read (-1: none, s outside [pos[0], pos[n - 1]))."""
    pos = np.asarray(pos, dtype=np.float64)
    s = np.atleast_1d(np.asarray(s, dtype=np.float64))
    n = len(pos)
    first, last = pos[0], pos[-1]
    ub = np.where(s < first, 0, n).astype(np.int64)   # rp_device.h:164 (NaN -> n)
    vmin = np.full(s.shape, n, dtype=np.int64)
    vmax = np.full(s.shape, -1, dtype=np.int64)
    b_read = np.full(s.shape, -1, dtype=np.int64)

    def touch(idx, where):
        np.minimum(vmin, np.where(where, idx, n), out=vmin)
        np.maximum(vmax, np.where(where, idx, -1), out=vmax)

    m = (s >= first) & (s < last)                      # :165
    if m.any():
        assert bk.nb > 0, "no bucket table: the kernels search (upper_bound), which this restatement does not cover"
        sm = np.where(m, s, first)
        b = ((sm - first) * bk.inv_h).astype(np.int64)  # :166 (int) of a non-negative double: truncation
        b = np.where(b < bk.nb, b, bk.nb - 1)           # :167
        b_read = np.where(m, b, -1)
        u = bk.table[b].astype(np.int64)                # :168
        back = m & (u > 0)                              # :169 reads pos[ub - 1]
        touch(u - 1, back)
        u = np.where(back & (pos[np.maximum(u - 1, 0)] > sm), u - 1, u)
        for _ in range(2):                              # :170, :171 read pos[ub]
            fwd = m & (u < n)
            touch(u, fwd)
            u = np.where(fwd & ~(pos[np.minimum(u, n - 1)] > sm), u + 1, u)
        ub = np.where(m, u, ub)
    # rp_kernels.h lon_step_part: s_idx = ub == n ? -1 : ub - 1; k0 = s_idx < 0 ? n - 1 : s_idx; k1 = s_idx + 1
    s_idx = np.where(ub == n, -1, ub - 1)
    k0 = np.where(s_idx < 0, n - 1, s_idx)
    k1 = s_idx + 1
    every = np.ones(s.shape, dtype=bool)
    touch(k0, every)
    touch(k1, every)
    k = np.clip(ub - 1, 0, n - 2)                       # foot point: k, k + 1
    touch(k, every)
    touch(k + 1, every)
    return Reads(ub, vmin, vmax, b_read)


# ---- the plan's items -----------------------------------------------------------------------------------------------------------
def lon_coeffs(lon_mode, x0_lon, T, sample):
    """c0 .. c5 of the longitudinal polynomial of a (T, sample) pair: rp_device.h quartic_coeffs (velocity keeping, sample = target
    velocity) / quintic_coeffs (stopping, sample = target position, at rest).  Plain double arithmetic: the last bits may differ
    from the device's, which is why every classified item keeps a distance from the window's bounds."""
    p0, v0, a0 = (float(v) for v in x0_lon)
    T = np.asarray(T, dtype=np.float64)
    sample = np.asarray(sample, dtype=np.float64)
    z = np.zeros(np.broadcast(T, sample).shape)
    if lon_mode == LON_STOPPING:
        bp = sample - (p0 + v0 * T + 0.5 * a0 * T * T)
        bv = 0.0 - (v0 + a0 * T)
        ba = 0.0 - a0
        c3 = (20.0 * bp - 8.0 * T * bv + T * T * ba) / (2.0 * T ** 3)
        c4 = (-30.0 * bp + 14.0 * T * bv - 2.0 * T * T * ba) / (2.0 * T ** 4)
        c5 = (12.0 * bp - 6.0 * T * bv + T * T * ba) / (2.0 * T ** 5)
    else:
        bv = sample - v0 - a0 * T
        ba = -a0
        c3 = (3.0 * bv - T * ba) / (3.0 * T * T)
        c4 = (T * ba - 2.0 * bv) / (4.0 * T ** 3)
        c5 = z
    return np.stack((z + p0, z + v0, z + 0.5 * a0, c3 + z, c4 + z, c5 + z))


def poly_pos(c, t):
    return ((((c[5] * t + c[4]) * t + c[3]) * t + c[2]) * t + c[1]) * t + c[0]


def pair_positions(lon_mode, x0_lon, T, L, N, dt):
    """s of every item: [nT * nL pairs (pair = iT * nL + iL)][N + 1 steps]"""
    TT, LL = np.meshgrid(np.asarray(T, dtype=np.float64), np.asarray(L, dtype=np.float64), indexing="ij")
    c = lon_coeffs(lon_mode, x0_lon, TT.ravel(), LL.ravel())
    t = np.arange(N + 1, dtype=np.float64) * dt
    return poly_pos(c[:, :, None], t[None, :])


def workgroup_pairs(n_cand, nD, lanes, cand_begin=0):
    """(first pair, last pair) of every workgroup of a single-launch plan of candidates [cand_begin, cand_begin + n_cand)"""
    gpb = RP_BLOCK // lanes
    out = []
    for b in range((n_cand + gpb - 1) // gpb):
        first = cand_begin + b * gpb
        last = cand_begin + min(n_cand, (b + 1) * gpb) - 1
        out.append((first // nD, last // nD))
    return out


Classes = collections.namedtuple("Classes", "inside outside margin")   # workgroup counts; smallest distance of an item's s to a bound


def classify(pos, win: Window, lon_mode, x0_lon, T, L, nD, N, dt, lanes, cand_begin=0, n_cand=None):
    """Workgroups of the plan without / with an item outside [win_s_lo, win_s_hi), from the prologue's own item set; and per
    workgroup the flag (True: some item outside)."""
    S = pair_positions(lon_mode, x0_lon, T, L, N, dt)
    if n_cand is None:
        n_cand = len(T) * len(L) * nD - cand_begin
    out_item = ~((S >= win.s_lo) & (S < win.s_hi))
    margin = float(np.min(np.minimum(np.abs(S - win.s_lo), np.abs(S - win.s_hi)))) if S.size else np.inf
    flags = [bool(out_item[p0:p1 + 1].any()) for p0, p1 in workgroup_pairs(n_cand, nD, lanes, cand_begin)]
    return Classes(flags.count(False), flags.count(True), margin), flags
