"""Exact kinematic verdicts at their thresholds (TEST INFRASTRUCTURE: tests/test_kin_abi.py on the CPU, tests/test_kin.py on the GPU).

TRUTH: the real-number inequalities of ``ReactivePlanner._check_constraints`` that the DOUBLE inputs define, evaluated in the
double-word longdouble arithmetic of tests/_dd.py.  Every check yields a signed margin g, the check fails when g < 0:
  velocity       g = v + 1e-5                                            (the double 1e-5)
  kappa          g = tan(delta_max) / wheelbase - |kappa|                (the tangent of the double delta_max, in extended precision)
  yaw rate       r = round-half-even((theta_i - theta_{i-1}) / dt * 1e5),  g = kappa_max v - |r| / 1e5
                 second edge: the half-integers of yaw * 1e5, margin = their distance to yaw * 1e5 in the yaw rate's units
  kappa_dot      g = v_delta_max (1 + (wheelbase kappa)^2) / wheelbase - |(kappa_i - kappa_{i-1}) / dt|
  acceleration   g = min(a + a_max, hi - a),  hi = a_max v_switch / v above v_switch, else a_max
both rates are 0 at step 0.  The verdict: the first step with a failing enabled check, then the first failing check in that order.

GUARD BAND  B = 16 u scale, u = 2^-53, scale = the magnitudes of the bound and of the terms that form the checked quantity, summed (for
the rates: the two neighbours divided by dt).  B is not taken from the device: tests/test_kin_abi.py measures the largest |g| at which
the double restatements (tests/_score.check_constraints, oracle/rp_oracle.c) decide otherwise than this reference and asserts that
B is at least 8 times that.

THE CASES (tier 1, the scorer; tier 2 feeds the rows whose theta is constant through the lift, where v = s_dot, a = s_ddot and
kappa = d_ddot on a straight path in low-velocity mode with d_dot = 0).  A case is one trajectory.  A family places ONE margin at
+-64 B, +-2^16 B and +-1e-6 scale ("+": passes, "-": fails at the step it names), the inputs are rounded to doubles and the margin is
recomputed from those doubles: |g| >= 8 B with the intended sign, every other margin of every step >= 1e-6 scale -- conditions on the
generator (asserted, never a reason to drop a case).  Bounds without rounding (``exact``: v at -1e-5, a at +-a_max, v at v_switch,
v = 0 with yaw = 0) need no guard: the bound itself passes and the doubles beside it decide.  Rows marked ``doc`` (exact ties of the
documented double arithmetic rint(x * 1e5) / 1e5, non-finite inputs) are held to the arithmetic include/rp_score.h states, restated in
NumPy (``documented``), not to the real-number reference.
Families: v_edge a_edge kappa acc_switch kappa_dot yaw_bound yaw_half yaw_tie where priority nonfinite.
Rows of every family but ``where`` end before pose N_POSES - 1 and are filled behind their end with the NEXT row's first pose, so that a
rate that reads its predecessor across a trajectory's first pose is seen in ``where`` alone (whose rows are filled with violations).

usage: python tests/_kin.py [out_file]      writes profiles/accuracy_kinematic.txt (on a GPU box: with the device's verdicts)"""
import functools
import math
import os
import sys
import time
from types import SimpleNamespace as NS

import numpy as np

if __name__ == "__main__":   # (as a script: the paths tests/conftest.py sets up for the suite)
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "commonroad-reactive-planner_amd"), os.path.join(_repo, "tests")]

import _dd as dd
from _dd import DD
from _xref import HAVE_LONGDOUBLE, SKIP_REASON   # noqa: F401  (what the tests skip with)
import _score as S

from commonroad_rp_amd._capi import copy_params

LD = np.longdouble
U = 2.0 ** -53
BAND = 16.0                  # B = BAND u scale
DECIDED = 8.0                # the placed margin: |g| >= DECIDED B
OTHER = 1e-6                 # every other margin: |g| >= OTHER scale
CHECKS = ("velocity", "kappa", "yaw_rate", "kappa_dot", "acceleration")   # the reference's order
BIT, REASON = S.CHECK, S.REASON
FULL = 31
LEVELS = (("64B", 64.0, None), ("65536B", 65536.0, None), ("1e-6", None, 1e-6))
N_POSES = 130
STEPS = (0, 1, 63, 64, 65, 127, 128)
FAMILIES = ("v_edge", "a_edge", "kappa", "acc_switch", "kappa_dot", "yaw_bound", "yaw_half", "yaw_tie", "where", "priority", "nonfinite")
LIFT_FAMILIES = ("v_edge", "a_edge", "kappa", "acc_switch", "kappa_dot")
PAIRS = tuple((a, b) for q, a in enumerate(CHECKS) for b in CHECKS[q + 1:])
MASKS = (FULL,) + tuple(BIT[c] for c in CHECKS) + tuple(FULL & ~BIT[c] for c in CHECKS) + tuple(BIT[a] | BIT[b] for a, b in PAIRS)
LIFT_MASKS = MASKS[:11]
TAN_SEED = 7                 # the draw of delta_max for which math.tan and np.tan differ starts here


# ---- the vehicle ---------------------------------------------------------------------------------------------------------------
def _vehicle(p, delta_max=None):
    return NS(dt=float(p.dt), wheelbase=float(p.wheelbase), a_max=float(p.a_max), v_switch=float(p.v_switch),
              delta_max=float(p.delta_max if delta_max is None else delta_max), v_delta_max=float(p.v_delta_max))


@functools.lru_cache(maxsize=None)
def tan_delta():
    """A delta_max in (0.2, 1.3) whose tangent libm and NumPy round differently (None: there is none among 20 000 draws here)."""
    rng = np.random.default_rng(TAN_SEED)
    for x in rng.uniform(0.2, 1.3, 20000):
        if math.tan(x) != float(np.tan(x)):
            return float(x)
    return None


@functools.lru_cache(maxsize=None)
def vehicles():
    p = S.fixture("cfg2_ref_draw").p
    out = {"std": _vehicle(p)}
    if tan_delta() is not None:
        out["tan"] = _vehicle(p, tan_delta())
    return out


def params_of(veh, mask):
    p = copy_params(S.fixture("cfg2_ref_draw").p)
    p.delta_max, p.constraint_mask = veh.delta_max, int(mask)
    return p


def kappa_max_dd(veh):
    s, c = dd.sincos(DD(LD(veh.delta_max)))
    return (s / c) / DD(LD(veh.wheelbase))


# ---- the exact reference ---------------------------------------------------------------------------------------------------------
def _prev(a):
    """the step before along the last axis (step 0: itself)"""
    return np.concatenate((a[..., :1], a[..., :-1]), axis=-1)


def exact(veh, v, a, kappa, theta):
    """Margins of [K, n] double inputs (all finite).  g[check]: longdouble, fail[check]: decided in double-word arithmetic,
    scale[check]: float64; half: distance of yaw * 1e5 to the nearest half-integer in the yaw rate's units; yaw_firm: the verdict of
    the yaw-rate bound is the same for r - 1, r and r + 1, each by OTHER scale."""
    raw = [np.atleast_2d(np.asarray(q)) for q in (v, a, kappa, theta)]           # doubles, or longdouble rows of tests/_xref.py
    V, A, Kp, Th = (DD(q.astype(LD)) for q in raw)
    v, a, kappa, theta = (q.astype(np.float64) for q in raw)                      # (for the scales)
    first = np.zeros(v.shape, bool)
    first[..., 0] = True
    dt, wb, amax, vsw, vdm = (DD(LD(q)) for q in (veh.dt, veh.wheelbase, veh.a_max, veh.v_switch, veh.v_delta_max))
    kmax, e5 = kappa_max_dd(veh), DD(LD(100000.0))
    kmax_f = float(kmax.ld())
    g, scale = {}, {}
    g["velocity"] = V + DD(LD(1e-5))
    scale["velocity"] = np.abs(v) + 1e-5
    g["kappa"] = kmax - abs(Kp)
    scale["kappa"] = kmax_f + np.abs(kappa)
    # yaw rate
    thp = _prev(theta)
    y = ((Th - DD(_prev(raw[3].astype(LD)))) / dt) * e5
    y = dd.where(first, dd.zeros(v.shape), y)
    f = np.floor(y.hi)
    frac = y - DD(f)
    low = frac < 0
    f, frac = np.where(low, f - 1, f), dd.where(low, frac + 1, frac)
    high = frac >= 1
    f, frac = np.where(high, f + 1, f), dd.where(high, frac - 1, frac)
    off = frac - DD(LD(0.5))
    tie = (off.hi == 0) & (off.lo == 0)
    r = f + np.where(tie, np.mod(f, 2), np.where(off > 0, 1, 0))
    bound = kmax * V
    g["yaw_rate"] = bound - DD(np.abs(r)) / e5
    scale["yaw_rate"] = kmax_f * np.abs(v) + np.where(first, 0.0, (np.abs(theta) + np.abs(thp)) / veh.dt)
    half = (abs(off) / e5).ld()
    alt = [(bound - DD(np.abs(r + q)) / e5).ld() for q in (-1, 0, 1)]
    firm = np.ones(v.shape, bool)
    for q in alt:
        firm &= (np.sign(q) == np.sign(alt[1])) & (np.abs(q) >= OTHER * scale["yaw_rate"])
    # kappa_dot
    kpp = _prev(kappa)
    wk = wb * Kp
    kd_bound = vdm * (DD(LD(1.0)) + wk * wk) / wb
    kd = dd.where(first, dd.zeros(v.shape), (Kp - DD(_prev(raw[2].astype(LD)))) / dt)
    g["kappa_dot"] = kd_bound - abs(kd)
    scale["kappa_dot"] = np.asarray(kd_bound.ld(), dtype=np.float64) + np.where(first, 0.0, (np.abs(kappa) + np.abs(kpp)) / veh.dt)
    # acceleration
    above = V > vsw
    hi = dd.where(above, amax * vsw / dd.where(above, V, DD(np.ones(v.shape, dtype=LD))), dd.broadcast_to(amax, v.shape))
    lo_side, hi_side = A + amax, hi - A
    lower = lo_side < hi_side
    g["acceleration"] = dd.where(lower, lo_side, hi_side)
    scale["acceleration"] = np.where(lower, veh.a_max, np.asarray(hi.ld(), dtype=np.float64)) + np.abs(a)
    fail = {c: np.asarray(g[c] < 0) for c in CHECKS}
    return NS(g={c: g[c].ld() for c in CHECKS}, fail=fail, scale=scale, half=half, yaw_firm=firm, r=r)


def documented(veh, v, a, kappa, theta, defect=None):
    """fail[check] [K, n] of the arithmetic include/rp_score.h states, in NumPy doubles.  ``defect`` plants one of DEFECTS."""
    v, a, kappa, theta = (np.atleast_2d(np.asarray(q, dtype=np.float64)) for q in (v, a, kappa, theta))
    first = np.zeros(v.shape, bool)
    first[..., 0] = True
    kmax = math.tan(veh.delta_max) / veh.wheelbase
    if defect == "kappa_max_float32":
        kmax = float(np.float32(kmax))
    gt = np.greater_equal if defect == "ge_for_gt" else np.greater
    with np.errstate(all="ignore"):
        fail = {"velocity": v < 0 if defect == "v_below_zero" else v <= -1e-5 if defect == "ge_for_gt" else v < -1e-5, "kappa": gt(np.abs(kappa), kmax)}
        yaw = np.where(first, 0.0, (theta - _prev(theta)) / veh.dt)
        x = yaw * 1e5
        rnd = {"trunc_for_rint": np.trunc, "half_away_for_rint": lambda q: np.sign(q) * np.floor(np.abs(q) + 0.5)}.get(defect, np.rint)
        fail["yaw_rate"] = gt(np.abs(rnd(x) / 1e5), kmax * v)
        wk = veh.wheelbase * kappa
        kd = np.where(first, 0.0, (kappa - _prev(kappa)) / veh.dt)
        fail["kappa_dot"] = gt(np.abs(kd), veh.v_delta_max * (1.0 + wk * wk) / veh.wheelbase)
        if defect == "reciprocal_float32":
            above = veh.a_max * veh.v_switch * np.float32(1.0 / v).astype(np.float64)
        else:
            above = veh.a_max * veh.v_switch / v
        hi = np.where(v > veh.v_switch, above, veh.a_max)
        ok = (-veh.a_max < a) & (a < hi) if defect == "ge_for_gt" else (-veh.a_max <= a) & (a <= hi)
        fail["acceleration"] = ~ok
    if defect == "rates_from_predecessor":   # step 0 of trajectory k > 0 reads the pose in front of it in memory
        th_p, kp_p = np.roll(theta.ravel(), 1).reshape(theta.shape), np.roll(kappa.ravel(), 1).reshape(kappa.shape)
        with np.errstate(all="ignore"):
            yaw0 = (theta - th_p) / veh.dt
            kd0 = (kappa - kp_p) / veh.dt
            wk = veh.wheelbase * kappa
            later = first.copy()
            later[0] = False
            fail["yaw_rate"] = np.where(later, np.abs(np.rint(yaw0 * 1e5) / 1e5) > kmax * v, fail["yaw_rate"])
            fail["kappa_dot"] = np.where(later, np.abs(kd0) > veh.v_delta_max * (1.0 + wk * wk) / veh.wheelbase, fail["kappa_dot"])
    return fail


DEFECTS = ("ge_for_gt", "v_below_zero", "kappa_max_float32", "trunc_for_rint", "half_away_for_rint", "reciprocal_float32", "reversed_chain",
           "rates_from_predecessor")


def status_words(fail, lengths, mask, reverse=False):
    """[K] uint32 status words of per-step failures under a mask: the first failing step, there the first failing check"""
    K, n = fail["velocity"].shape
    code = np.zeros((K, n), dtype=np.int64)
    for c in (CHECKS if reverse else CHECKS[::-1]):   # (the earliest check is written last)
        if mask & BIT[c]:
            code = np.where(fail[c], REASON[c], code)
    code[np.arange(n)[None, :] >= np.asarray(lengths)[:, None]] = 0
    bad = code != 0
    step = bad.argmax(axis=1)
    reason = code[np.arange(K), step]
    return np.where(bad.any(axis=1), 2 | (reason << 4) | (step << 8), 1).astype(np.uint32)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
class _Rows:
    def __init__(self, veh):
        self.veh = veh
        self.kmax = kappa_max_dd(veh).ld().reshape(())[()]
        self.rows = []
        self._step = 0

    def step(self, lowest=0):
        """the deciding steps in turn"""
        while True:
            s = STEPS[self._step % len(STEPS)]
            self._step += 1
            if s >= lowest:
                return s

    def new(self, family, sign, level, step, L=None, **kw):
        veh = self.veh
        L = min(N_POSES - 1, step + 1 + (len(self.rows) % 5)) if L is None else L
        r = NS(family=family, sign=sign, level=level, step=step, L=L, placed=set(), exact=False, doc=False, delta=math.nan,
               v=np.full(N_POSES, 0.5 * veh.v_switch), a=np.full(N_POSES, 0.25 * veh.a_max), kappa=np.full(N_POSES, 0.01 * float(self.kmax)),
               theta=np.zeros(N_POSES), **kw)
        self.rows.append(r)
        return r

    def delta(self, level, scale):
        _, times_b, rel = level
        return LD(times_b * BAND * U) * LD(scale) if rel is None else LD(rel) * LD(scale)


def _both(level_list=LEVELS):
    for level in level_list:
        for sign in (+1, -1):
            yield level, sign


def _build_rows(veh, families):
    R = _Rows(veh)
    kmax, dt, amax, vsw, wb, vdm = R.kmax, LD(veh.dt), LD(veh.a_max), LD(veh.v_switch), LD(veh.wheelbase), LD(veh.v_delta_max)
    nxt = np.nextafter
    if "v_edge" in families:
        for val, sign in ((-1e-5, +1), (nxt(-1e-5, -1.0), -1), (nxt(-1e-5, 0.0), +1)):
            r = R.new("v_edge", sign, "ulp", R.step())
            r.v[r.step], r.exact = val, True
            r.placed.add((r.step, "velocity"))
    if "a_edge" in families:
        for val, sign in ((veh.a_max, +1), (nxt(veh.a_max, 99.0), -1), (nxt(veh.a_max, 0.0), +1), (-veh.a_max, +1), (nxt(-veh.a_max, -99.0), -1),
                          (nxt(-veh.a_max, 0.0), +1)):
            r = R.new("a_edge", sign, "ulp", R.step())
            r.a[r.step], r.exact = val, True
            r.placed.add((r.step, "acceleration"))
        for val, sign in ((veh.a_max, +1), (nxt(veh.a_max, 99.0), -1)):   # v == v_switch: ">" keeps the plain a_max
            r = R.new("a_edge", sign, "ulp", R.step())
            r.a[r.step], r.v[r.step], r.exact = val, veh.v_switch, True
            r.placed.add((r.step, "acceleration"))
    if "kappa" in families:
        for sgn in (+1, -1):
            for level, sign in _both():
                r = R.new("kappa", sign, level[0], R.step())
                r.delta = R.delta(level, 2 * kmax)
                r.kappa[:] = float(sgn * kmax * LD(1 - 1e-3))
                r.kappa[r.step:] = float(sgn * (kmax - sign * r.delta))
                r.placed |= {(j, "kappa") for j in range(r.step, N_POSES)}
    if "acc_switch" in families:
        for vv in (veh.v_switch * (1 + 1e-9), veh.v_switch * 1.001, veh.v_switch * 1.5, 20.0, 40.0):
            hi = amax * vsw / LD(vv)
            for level, sign in _both():
                r = R.new("acc_switch", sign, level[0], R.step())
                r.delta = R.delta(level, 2 * hi)
                r.v[r.step], r.a[r.step] = vv, float(hi - sign * r.delta)
                r.placed.add((r.step, "acceleration"))
        for vv in (veh.v_switch * 1.5, 40.0):                              # the lower limit does not move with v
            for level, sign in _both():
                r = R.new("acc_switch", sign, level[0], R.step())
                r.delta = R.delta(level, 2 * amax)
                r.v[r.step], r.a[r.step] = vv, float(-amax + sign * r.delta)
                r.placed.add((r.step, "acceleration"))
        for vv, sign in ((veh.v_switch * (1 - 1e-9), +1), (veh.v_switch * (1 + 1e-9), -1)):   # the branch edge: a between the two limits
            r = R.new("acc_switch", sign, "branch", R.step())
            r.v[r.step], r.a[r.step] = vv, veh.a_max * (1 - 0.5e-9)
            r.placed.add((r.step, "acceleration"))
    if "kappa_dot" in families:
        for wk in (0.0, 0.5, 1.5, 3.0):
            for rising in (True, False):
                k_i = np.float64(wk / veh.wheelbase) * (1.0 if rising else -1.0)
                bound = vdm * (1 + (wb * LD(k_i)) ** 2) / wb
                for level, sign in _both():
                    r = R.new("kappa_dot", sign, level[0], R.step(1))
                    k_p = LD(k_i) - (1 if rising else -1) * dt * bound
                    r.delta = R.delta(level, bound + (abs(LD(k_i)) + abs(k_p)) / dt)
                    k_p = LD(k_i) - (1 if rising else -1) * dt * (bound - sign * r.delta)
                    r.kappa[:r.step], r.kappa[r.step:] = float(k_p), k_i
                    r.placed.add((r.step, "kappa_dot"))
    if "yaw_bound" in families:
        r = R.new("yaw_bound", +1, "zero", R.step(1))                      # v = 0, yaw = 0: 0 > 0, no rounding anywhere
        r.v[r.step], r.exact = 0.0, True
        r.placed.add((r.step, "yaw_rate"))
        for rr in (1, 7, 250, 4001):
            for sgn in (+1, -1):
                for level, sign in _both():
                    r = R.new("yaw_bound", sign, level[0], R.step(1))
                    th0 = 0.001 if rr == 7 else 0.0
                    th1 = th0 + sgn * veh.dt * rr / 1e5
                    bound = LD(rr) / LD(100000.0)
                    r.delta = R.delta(level, bound + (abs(th0) + abs(th1)) / veh.dt)
                    r.theta[:r.step], r.theta[r.step:] = th0, th1
                    r.v[r.step] = float((bound + sign * r.delta) / kmax)
                    r.placed.add((r.step, "yaw_rate"))
    if "yaw_half" in families:
        for k in (0, 1, 6, 7, 250, 4001):
            for sgn in (+1, -1):
                for level, sign in _both():
                    r = R.new("yaw_half", sign, level[0], R.step(1))
                    mid = (LD(k) + LD(0.5)) / LD(100000.0)
                    r.delta = R.delta(level, 2 * mid)
                    r.theta[r.step:] = float(sgn * dt * (mid - sign * r.delta))
                    r.v[r.step] = float(mid / kmax)                       # r = k passes, r = k + 1 fails
                    r.placed.add((r.step, "yaw_half"))
    if "yaw_tie" in families:
        def tie_theta(k):
            """a double theta with fl(fl(theta / dt) 1e5) == k + 0.5 exactly, or None (the two roundings skip about half of the k)"""
            up = down = np.float64((k + 0.5) * 1e-5 * veh.dt)
            for _ in range(8):
                for c in (up, down):
                    if (c / veh.dt) * 1e5 == k + 0.5:
                        return c
                up, down = nxt(up, 1.0), nxt(down, 0.0)
            return None
        for base in (2, 3, 250, 251, 4000, 4001):   # the first k of either parity from here on that such a theta exists for
            k = next(q for q in range(base, base + 400, 2) if tie_theta(q) is not None)
            for sgn in (+1, -1):
                r = R.new("yaw_tie", +1 if k % 2 == 0 else -1, f"tie {k}.5", R.step(1))
                r.theta[r.step:] = sgn * tie_theta(k)
                r.v[r.step], r.doc = float(((LD(k) + LD(0.5)) / LD(100000.0)) / kmax), True
    if "where" in families:
        bad_kappa = 1.5 * float(kmax)
        for s in STEPS:
            for what in ("kappa", "yaw_rate", "kappa_dot"):
                if s == 0 and what != "kappa":
                    continue
                r = R.new("where", -1, what, s, L=min(N_POSES, s + 2))
                if what == "kappa":
                    r.kappa[s] = bad_kappa
                elif what == "yaw_rate":
                    r.theta[s:] += 0.6
                else:
                    r.kappa[s:] += 0.05
        for L in (1, 64, 65, 129, 130):                                    # the last pose decides
            r = R.new("where", -1, "last", L - 1, L=L)
            r.a[L - 1] = 2 * veh.a_max
        for L in (1, 63, 64, 65, 128, 129, 130):                           # what stands behind the end decides nothing
            R.new("where", +1, "behind", L - 1, L=L)
    if "priority" in families:
        def atom(r, c, s):
            if c == "velocity":
                r.v[s] = -0.5
            elif c == "kappa":
                r.kappa[s] += 1.5 * float(kmax)
            elif c == "yaw_rate":
                r.theta[s:] += 0.6
            elif c == "kappa_dot":
                r.kappa[s:] += 0.05
            else:
                r.a[s] = 2 * veh.a_max
        for a_, b_ in PAIRS:                                               # both in one step
            r = R.new("priority", -1, f"{a_}+{b_}", R.step(1), pair=(a_, b_))
            atom(r, a_, r.step)
            atom(r, b_, r.step)
        for a_, b_ in PAIRS:                                               # the later check fails first, and the other way round
            for early, late in ((b_, a_), (a_, b_)):
                s = min(R.step(1), N_POSES - 6)
                r = R.new("priority", -1, f"{early}>{late}", s, L=min(N_POSES - 1, s + 8), pair=(a_, b_))
                atom(r, early, s)
                atom(r, late, s + 3)
    if "nonfinite" in families:
        for var in ("v", "a", "kappa", "theta"):
            for val in (math.nan, math.inf, -math.inf):
                r = R.new("nonfinite", -1, f"{var}={val}", R.step(1))
                getattr(r, var)[r.step] = val
                r.doc = True
        for val in (1e200, -1e200):   # finite, but 1 + (wheelbase kappa)^2 overflows: inf > inf passes kappa_dot at that step
            r = R.new("nonfinite", -1, f"kappa={val}", R.step(1))
            r.kappa[r.step], r.doc = val, True
    return R.rows


@functools.lru_cache(maxsize=None)
def group(name, lift=False):
    """The rows of a vehicle as arrays [K, N_POSES] with their lengths, and the reference's answer under every mask."""
    veh = vehicles()[name]
    fams = LIFT_FAMILIES if lift else FAMILIES if name == "std" else ("kappa", "yaw_bound")
    rows = _build_rows(veh, fams)
    rows.sort(key=lambda r: r.family == "where")          # (stable: ``where`` last)
    K = len(rows)
    v, a, kappa, theta = (np.stack([getattr(r, q) for r in rows]) for q in ("v", "a", "kappa", "theta"))
    lengths = np.array([r.L for r in rows], dtype=np.int32)
    for k, r in enumerate(rows):                           # behind the end
        if r.family == "where":
            v[k, r.L:], a[k, r.L:], kappa[k, r.L:], theta[k, r.L:] = -5.0, 100.0, 50.0, 2.0
        else:
            assert r.L < N_POSES
            nk = (k + 1) % K
            theta[k, r.L:], kappa[k, r.L:] = theta[nk, 0], kappa[nk, 0]
    if lift:
        theta = np.zeros_like(theta)
        v = np.where(np.abs(v) < 1e-5, 0.0, v)             # the lift's own rule for s_dot, applied to its expected v
    family = np.array([r.family for r in rows])
    doc = np.array([r.doc for r in rows])
    ex = exact(veh, *(np.where(doc[:, None], 0.0, q) for q in (v, a, kappa, theta)))   # (``doc`` rows: not the real-number reference's)
    docf = documented(veh, v, a, kappa, theta)
    fail = {c: np.where(doc[:, None], docf[c], ex.fail[c]) for c in CHECKS}
    want = {m: status_words(fail, lengths, m) for m in MASKS}
    g = NS(name=name, veh=veh, rows=rows, K=K, v=v, a=a, kappa=kappa, theta=theta, lengths=lengths, family=family, doc=doc, exact=ex, fail=fail,
           want=want, sign=np.array([r.sign for r in rows]), step=np.array([r.step for r in rows]))
    # poses on the straight two-vertex path of tests/_score.py: s advancing, every trajectory at its own small offset
    ref, pos, th = S.path("two_vertex")
    h = th[0]
    s = 5.0 + 0.05 * np.arange(N_POSES)[None, :] + np.zeros((K, 1))
    d = (-1.0 + 2.0 * np.arange(K) / K)[:, None] + np.zeros((1, N_POSES))
    g.s, g.d = s, d
    g.x, g.y = ref[0, 0] + s * math.cos(h) - d * math.sin(h), ref[0, 1] + s * math.sin(h) + d * math.cos(h)
    for q in (g.v, g.a, g.kappa, g.theta, g.lengths, g.x, g.y, g.s, g.d):
        q.setflags(write=False)
    return g


def score_rows(g):
    return dict(x=g.x, y=g.y, theta=g.theta, v=g.v, a=g.a, kappa=g.kappa, lengths=g.lengths)


def margin_failures(g):
    """Rows that do not meet the conditions of a case: [(row, family, step, check, g, bound)].  Empty for a sound generator."""
    out = []
    ex = g.exact
    live = np.arange(N_POSES)[None, :] < g.lengths[:, None]
    for k, r in enumerate(g.rows):
        if r.doc:
            continue
        for c in CHECKS:
            mg, sc = np.abs(ex.g[c][k]).astype(np.float64), ex.scale[c][k]
            for j in np.flatnonzero(live[k]):
                placed = (j, c) in r.placed
                if c == "yaw_rate" and not placed:
                    half_placed = (j, "yaw_half") in r.placed
                    if half_placed:
                        need = DECIDED * BAND * U * sc[j]
                        if not float(ex.half[k, j]) >= need:
                            out.append((k, r.family, j, "yaw_half", float(ex.half[k, j]), need))
                        if not mg[j] >= OTHER * sc[j]:
                            out.append((k, r.family, j, c, mg[j], OTHER * sc[j]))
                    elif not (ex.yaw_firm[k, j] or float(ex.half[k, j]) >= OTHER * sc[j] and mg[j] >= OTHER * sc[j]):
                        out.append((k, r.family, j, c, mg[j], OTHER * sc[j]))
                    continue
                need = 0.0 if (placed and r.exact) else DECIDED * BAND * U * sc[j] if placed else OTHER * sc[j]
                if not mg[j] >= need:
                    out.append((k, r.family, j, c, mg[j], need))
    return out


def own_check(r):
    return {"v_edge": "velocity", "a_edge": "acceleration", "kappa": "kappa", "acc_switch": "acceleration", "kappa_dot": "kappa_dot",
            "yaw_bound": "yaw_rate", "yaw_half": "yaw_rate", "yaw_tie": "yaw_rate"}.get(r.family)


@functools.lru_cache(maxsize=None)
def costs(name):
    """The reference's cost of every row (constraint mask 0: all of them feasible), for ``best``"""
    g = group(name)
    f = S.fixture("cfg2_ref_draw")
    ref, pos, th = S.path("two_vertex")
    with np.errstate(all="ignore"):
        return S.reference(params_of(g.veh, 0), f.cost, ref, pos, th, **score_rows(g)).cost


def selection(g, mask):
    """(best, n_feasible, reason_counts) the status words of a mask imply"""
    st = g.want[mask]
    c = costs(g.name)
    feas = np.flatnonzero(st == 1)
    best = -1
    for k in feas:
        if c[k] == c[k] and (best < 0 or c[k] < c[best]):
            best = int(k)
    counts = np.bincount((st[st != 1] >> 4) & 7, minlength=8).astype(np.int64)
    return best, int(feas.size), counts


def runner_up_gap(g, mask):
    """relative distance of the two cheapest feasible costs: the choice of ``best`` must not hang on the cost's rounding"""
    c = np.sort(costs(g.name)[(g.want[mask] == 1)])
    c = c[np.isfinite(c)]
    return math.inf if c.size < 2 else float((c[1] - c[0]) / abs(c[0]))


# ---- the lift (tier 2): the same rows as s_dot, s_ddot, d_ddot on a straight path ------------------------------------------------
LIFT_POINTS = ((3.0, -2.0), (83.0, 38.0))


def lift_inputs(g, raw_v):
    """the six planes; ``raw_v``: the rows' v BEFORE the lift's |s_dot| < 1e-5 rule (group(..., lift=True).v is what it must become)"""
    z = np.zeros_like(g.s)
    return dict(s=g.s, s_dot=raw_v, s_ddot=g.a, d=g.d, d_dot=z, d_ddot=g.kappa, lengths=g.lengths)


@functools.lru_cache(maxsize=None)
def lift_raw_v(name="std"):
    rows = _build_rows(vehicles()[name], LIFT_FAMILIES)
    return np.stack([r.v for r in rows])


# ---- the lift's input branch edges: no guard, the doubles beside an edge decide ---------------------------------------------------
EDGE_POSES = (1, 63, 64, 65)
EDGE_N = 80


def _edge_values():
    nx = np.nextafter
    sd = [1e-5, nx(1e-5, 0.0), nx(1e-5, 1.0), -1e-5, nx(-1e-5, 0.0), nx(-1e-5, -1.0), 0.001, nx(0.001, 1.0), nx(0.001, 0.0)]
    dd = [1e-5, nx(1e-5, 0.0), nx(1e-5, 1.0), -1e-5, nx(-1e-5, 0.0), nx(-1e-5, -1.0)]
    return sd, dd


@functools.lru_cache(maxsize=None)
def lift_edges():
    """Trajectories on the curved path of the cfg2 fixture in high-velocity mode that move at 3 m/s and, from pose q of EDGE_POSES on, hold
    s_dot at an edge of the lift's input rules (|s_dot| < 1e-5 reads as 0; s_dot > 0.001 moves) -- a standstill carry that starts on
    the edge pose, for q = 63 on the last lane of a chunk -- or have d_dot on such an edge at that pose alone; with the NumPy reference's
    answer (tests/_lift.py)."""
    import _lift
    f = S.fixture("cfg2_ref_draw")
    t = _lift.fixture_path("cfg2_ref_draw")
    p = copy_params(f.p)
    p.low_vel_mode, p.constraint_mask = 0, FULL
    sd_edges, dd_edges = _edge_values()
    rows = []
    for q in EDGE_POSES:
        for val in sd_edges:
            sd = np.full(EDGE_N, 3.0)
            sd[q:] = val
            rows.append((q, "s_dot", val, sd, np.full(EDGE_N, 0.01)))
        for val in dd_edges:
            dd_ = np.full(EDGE_N, 0.01)
            dd_[q] = val
            rows.append((q, "d_dot", val, np.full(EDGE_N, 3.0), dd_))
    K = len(rows)
    sd, dd_ = np.stack([r[3] for r in rows]), np.stack([r[4] for r in rows])
    s = t.pos[0] + 0.1 * (t.pos[-1] - t.pos[0]) + np.concatenate((np.zeros((K, 1)), np.cumsum(np.maximum(sd, 0.0), 1)[:, :-1]), 1) * float(p.dt)
    d = np.full((K, EDGE_N), 1.5) + 0.001 * np.arange(K)[:, None]
    z = np.zeros((K, EDGE_N))
    lengths = np.array([EDGE_N - (k % 3) for k in range(K)], dtype=np.int32)
    planes = dict(s=s, s_dot=sd, s_ddot=z, d=d, d_dot=dd_, d_ddot=z)
    out = _lift.reference(p, t, lengths=lengths, **planes)
    return NS(p=p, path=t, planes=planes, lengths=lengths, out=out, what=[r[:3] for r in rows], K=K)


def lift_edge_margins(c):
    """the smallest |g| / scale of the reference's own rows of lift_edges() over the steps that have rows (a comparison of two zeros,
    0 > 0, involves no rounding and is left out; the GPU test asserts that a kept orientation is a copy on the device too)"""
    o = c.out
    live = ~np.isnan(o.theta)
    ex = exact(_vehicle(c.p), *(np.nan_to_num(q) for q in (o.v, o.a, o.kappa, o.theta)))
    worst = math.inf
    for ch in CHECKS:
        g, sc = np.abs(ex.g[ch]).astype(np.float64), ex.scale[ch]
        use = live & ~((g == 0) & (ch == "yaw_rate"))
        if ch == "yaw_rate":   # an orientation that is kept is a copy: its yaw rate is an exact 0, only kappa_max v is rounded
            sc = np.where(o.theta == _prev(o.theta), float(kappa_max_dd(_vehicle(c.p)).ld()) * np.abs(np.nan_to_num(o.v)), sc)
        worst = min(worst, float((g[use] / sc[use]).min()))
    return worst


# ---- the measurement behind B ----------------------------------------------------------------------------------------------------
LADDER = (0, 1, 2, 4, 8, 32)


def ladder(n_draws=6000, seed=11):
    """Random single-step configurations of every check, the checked quantity displaced by +-k u scale from its bound (k of LADDER):
    a group-like namespace of two-pose trajectories [K, 2] whose step 1 carries the check, and the check of every row."""
    veh = vehicles()["std"]
    rng = np.random.default_rng(seed)
    kmax = kappa_max_dd(veh).ld().reshape(())[()]
    dt, amax, vsw, wb, vdm = LD(veh.dt), LD(veh.a_max), LD(veh.v_switch), LD(veh.wheelbase), LD(veh.v_delta_max)
    rows, checks = [], []
    for c in ("kappa", "yaw_rate", "kappa_dot", "acceleration"):
        for _ in range(n_draws):
            k = LADDER[int(rng.integers(len(LADDER)))] * (1 if rng.random() < 0.5 else -1)
            v, a, kp, th = np.full(2, 0.5 * veh.v_switch), np.zeros(2), np.zeros(2), np.zeros(2)
            if c == "kappa":
                kp[:] = float((kmax + LD(k * U) * 2 * kmax) * (1 if rng.random() < 0.5 else -1))
            elif c == "yaw_rate":
                rr = int(rng.integers(1, 5000))
                th[0] = rng.uniform(-3.0, 3.0)
                th[1] = th[0] + (1 if rng.random() < 0.5 else -1) * veh.dt * rr / 1e5
                y = abs(LD(th[1]) - LD(th[0])) / dt
                scale = y + (abs(th[0]) + abs(th[1])) / veh.dt
                v[1] = float((LD(np.rint(float(y * 100000))) / 100000 + LD(k * U) * scale) / kmax)
            elif c == "kappa_dot":
                kp[1] = rng.uniform(-1.2, 1.2)
                bound = vdm * (1 + (wb * LD(kp[1])) ** 2) / wb
                sgn = 1 if rng.random() < 0.5 else -1
                k_p = LD(kp[1]) - sgn * dt * bound
                scale = bound + (abs(LD(kp[1])) + abs(k_p)) / dt
                kp[0] = float(LD(kp[1]) - sgn * dt * (bound + LD(k * U) * scale))
            else:
                v[1] = rng.uniform(veh.v_switch * 1.0001, 45.0)
                hi = amax * vsw / LD(v[1])
                a[1] = float(hi + LD(k * U) * 2 * hi)
            rows.append((v, a, kp, th))
            checks.append(c)
    v, a, kp, th = (np.stack([r[q] for r in rows]) for q in range(4))
    return NS(veh=veh, v=v, a=a, kappa=kp, theta=th, check=np.array(checks), exact=exact(veh, v, a, kp, th))


def worst_wrong_margin(lad, verdict_of):
    """{check: largest |g| / (u scale) over the ladder rows whose step-1 verdict by ``verdict_of(check, row index)`` (True: fails) differs
    from the reference's}"""
    out = {}
    for c in ("kappa", "yaw_rate", "kappa_dot", "acceleration"):
        worst = 0.0
        for k in np.flatnonzero(lad.check == c):
            if bool(verdict_of(c, k)) != bool(lad.exact.fail[c][k, 1]):
                worst = max(worst, float(abs(lad.exact.g[c][k, 1])) / (U * lad.exact.scale[c][k, 1]))
        out[c] = worst
    return out


def restatement_verdict(lad):
    def of(c, k):
        p = params_of(lad.veh, BIT[c])
        return S.check_constraints(p, lad.v[k], lad.kappa[k], lad.theta[k], lad.a[k], 1) != 0
    return of


def oracle_verdict(lad):
    from oracle import oracle

    def of(c, k):
        return oracle.step_reasons(params_of(lad.veh, BIT[c]), lad.v[k], lad.kappa[k], lad.theta[k], lad.a[k])[1] != 0
    return of


@functools.lru_cache(maxsize=None)
def measured():
    lad = ladder()
    return {"restatement": worst_wrong_margin(lad, restatement_verdict(lad)), "oracle": worst_wrong_margin(lad, oracle_verdict(lad)),
            "documented": worst_wrong_margin(lad, lambda c, k, f=documented(lad.veh, lad.v, lad.a, lad.kappa, lad.theta): f[c][k, 1])}


# ---- the device ----------------------------------------------------------------------------------------------------------------
def device_scorer(sc, g, mask):
    f = S.fixture("cfg2_ref_draw")
    return sc.score(params_of(g.veh, mask), f.cost, **score_rows(g))


def lift_params(veh, mask):
    p = params_of(veh, mask)
    p.low_vel_mode = 1
    return p


def device_results():
    """{(tier, group, mask): (got status, wanted status)}; a string that says why where there is no library or no device.  Only the import
    and the opening of the device are excused: a call that fails afterwards raises."""
    import _lift
    from commonroad_rp_amd._capi import RpError, RpLibraryMissing
    try:
        from commonroad_rp_amd import TrajectoryScorer
        from commonroad_rp_amd.lift import TrajectoryLifter
        sc, lf = TrajectoryScorer(0), TrajectoryLifter(0)
    except (ImportError, OSError, RpError, RpLibraryMissing) as e:
        return f"{type(e).__name__}: {e}"
    out = {}
    ref, pos, th = S.path("two_vertex")
    with sc, lf:
        sc.set_reference(ref, pos, th, 20.0)
        for name in vehicles():
            g = group(name)
            for m in MASKS:
                out[("scorer", name, m)] = (device_scorer(sc, g, m).status, g.want[m])
        g = group("std", lift=True)
        lf.set_reference(*_lift.table_args(_lift.built_path(LIFT_POINTS)))
        for m in LIFT_MASKS:
            out[("lift", "std", m)] = (lf.lift(lift_params(g.veh, m), **lift_inputs(g, lift_raw_v())).status, g.want[m])
        c = lift_edges()
        lf.set_reference(*_lift.table_args(c.path))
        out[("lift", "edge", FULL)] = (lf.lift(c.p, lengths=c.lengths, **c.planes).status, c.out.status)
    return out


def summary_lines(device=None):
    lines = ["Kinematic verdicts at their thresholds: tests/_kin.py against the exact reference (double-word longdouble).",
             f"B = {BAND:.0f} u scale, u = 2^-53; placed margins at +-64 B, +-2^16 B and +-1e-6 scale, each |g| >= {DECIDED:.0f} B after rounding;",
             f"every other margin >= {OTHER:.0e} scale.  delta_max with math.tan != np.tan: {tan_delta()!r}", ""]
    m = measured()
    lines.append("largest |g| [u scale] at which a double form decides otherwise than the reference (ladder of +-k u scale, k = 0 1 2 4 8 32):")
    for who in ("restatement", "oracle", "documented"):
        lines.append(f"  {who:12s} " + "  ".join(f"{c} {m[who][c]:.2f}" for c in m[who]))
    lines.append("")
    for tier, name, lift in (("1 scorer", "std", False), ("1 scorer", "tan", False), ("2 lift, exact placement", "std", True)):
        if name not in vehicles():
            continue
        g = group(name, lift)
        lines.append(f"tier {tier}, vehicle {name}: {g.K} trajectories of up to {N_POSES} poses, {len(LIFT_MASKS if lift else MASKS)} masks, "
                     f"{len(margin_failures(g))} rows outside the conditions of a case")
        for fam in FAMILIES:
            rows = [r for r in g.rows if r.family == fam]
            if not rows:
                continue
            dl = [float(r.delta) for r in rows if r.delta == r.delta]
            band = f"delta {min(dl):.2e} .. {max(dl):.2e}" if dl else "no guard (exact bounds, documented arithmetic or gross violations)"
            lines.append(f"  {fam:11s} {len(rows):4d} cases   {band}")
        lines.append("")
    c = lift_edges()
    lines += [f"tier 2 lift, input branch edges (s_dot at +-1e-5 and 0.001, d_dot at +-1e-5, the doubles beside them; from poses {EDGE_POSES} on): "
              f"{c.K} trajectories of up to {EDGE_N} poses against tests/_lift.py, smallest |g| / scale {lift_edge_margins(c):.1e}", ""]
    if isinstance(device, dict):
        lines.append("device verdicts (status words that differ from the reference's / compared):")
        for (tier, name, mask), (got, want) in device.items():
            bad = np.flatnonzero(got != want)
            lines.append(f"  {tier:7s} {name:4s} mask {mask:2d}: {len(bad)} / {len(want)}" + ("" if not len(bad) else f"   rows {list(bad[:8])}"))
    else:
        lines.append(f"device verdicts: not measured here ({device})")
    import _kin_plan as P   # (tiers 2, derived quantities, and 3: the vehicle limit placed against extended-precision rows)
    lines += [""] + P.summary_lines()
    if isinstance(device, dict):
        lines += [""] + P.device_lines()
    return lines


def main(argv):
    if not HAVE_LONGDOUBLE:
        print(SKIP_REASON)
        return 0
    t0 = time.time()
    out = argv[1] if len(argv) > 1 else os.path.join(S.REPO, "profiles", "accuracy_kinematic.txt")
    lines = summary_lines(device_results())
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(f"({time.time() - t0:.1f} s; written to {out})")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
