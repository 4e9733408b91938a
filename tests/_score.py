"""Shared by tests/test_score_abi.py (CPU) and tests/test_score.py (GPU): a NumPy reference of the scorer (include/rp_score.h) that
shares nothing with the device code, the inputs, and the reference's answers on them, computed once per session and never written to.

The reference: the projection is ``oracle.frontend.project`` with its loop over the points turned into array operations (segment by
segment, in ascending order, the two roots in that function's order, a candidate replacing the held one only when its |d| is strictly
smaller) so that it can also report the segment and lambda -- tests/test_score_abi.py holds it to ``oracle.frontend.project`` point by
point.  The constraints are ``ReactivePlanner._check_constraints`` with Python's ``round``, the costs the two default cost functions
with ``np.sum``."""
import functools
import math
import os
import re
from types import SimpleNamespace as NS

import numpy as np

from commonroad_rp_amd._capi import make_cost, make_params
from oracle import frontend

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rp_score.h")
SOURCE = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_score.hip")
GOLDEN = os.path.join(REPO, "tests", "golden")
_m = re.search(r"SC_LDS_ROWS\s*=\s*(\d+)", open(SOURCE).read()) if os.path.exists(SOURCE) else None
LDS_ROWS = int(_m.group(1)) if _m else 384   # segment rows the kernel stages in LDS; beyond: read from device memory

RP_X, RP_Y, RP_THETA, RP_V, RP_A, RP_KAPPA, RP_S, RP_D, RP_THETA_CL = 0, 1, 2, 3, 4, 5, 7, 8, 9
TOL = 1e-9         # metres / radians: the bound the project uses for lengths (tests/test_clearance.py)
COST_RTOL = 1e-12  # about a hundred times the rounding of a sum of up to 61 non-negative terms
EPS = 1e-5         # _EPS, reactive_planner.py:49
TWO_PI = 2.0 * np.pi

# the thirteen draw fixtures with states and L whose s stays on the path (short_path_ood_draw's runs past its end; corridor_arc_l1_draw
# has no L)
DRAW_FIXTURES = ("arc_hv_l1_draw", "arc_hv_standstill_draw", "cfg1_ref_l1_draw", "cfg1_ref_l1_rb_draw", "cfg1_ref_l2_draw", "cfg1_ref_l2_rb_draw",
                 "cfg1_ref_l3_draw", "cfg1_ref_l3_rb_draw", "cfg2_ref_draw", "cfg2_ref_rb_draw", "cfg3_ref_draw", "cfg3_ref_rb_draw", "scurve_lv_l1_draw")
GPU_FIXTURES = ("cfg1_ref_l1_draw", "cfg2_ref_draw", "arc_hv_standstill_draw", "scurve_lv_l1_draw")
U_PATH = np.array([[0.0, 0.0], [8.0, 0.0], [16.0, 0.0], [18.0, 2.0], [16.0, 4.0], [8.0, 4.0], [0.0, 4.0]])


# ---- the projection ----------------------------------------------------------------------------------------------------------
def project_batch(ref, ref_pos, x, y, d_limit=20.0, keep_candidates=False):
    """(s, d, segment, lambda) of points x, y (any shape): NaN, NaN, -1, NaN outside the projection domain.  With ``keep_candidates``
    also (|d|, s) of EVERY admissible candidate, [2 * segments, points] (NaN: none)."""
    ref, ref_pos = np.asarray(ref, float), np.asarray(ref_pos, float)
    shape = np.shape(x)
    x, y = np.asarray(x, float).ravel(), np.asarray(y, float).ravel()
    P = x.size
    tan = frontend.compute_vertex_tangents(ref)
    s, d, lam_out = np.full(P, np.nan), np.full(P, np.nan), np.full(P, np.nan)
    seg = np.full(P, -1)
    cand_ad = np.full((2 * (len(ref) - 1), P), np.nan) if keep_candidates else None
    cand_s = np.full((2 * (len(ref) - 1), P), np.nan) if keep_candidates else None
    with np.errstate(all="ignore"):
        for k in range(len(ref) - 1):
            ex, ey = ref[k + 1] - ref[k]
            qx, qy = x - ref[k, 0], y - ref[k, 1]
            t0x, t0y = tan[k]
            dtx, dty = tan[k + 1] - tan[k]
            a = -(ex * dtx + ey * dty)
            b = (qx * dtx + qy * dty) - (ex * t0x + ey * t0y)
            c = qx * t0x + qy * t0y
            if abs(a) < 1e-14:
                roots = [np.where(b != 0.0, -c / b, np.nan)]
            else:
                disc = b * b - 4.0 * a * c
                sq = np.sqrt(np.where(disc < 0.0, np.nan, disc))
                pos = b >= 0.0
                q = np.where(pos, -0.5 * (b + sq), -0.5 * (b - sq))
                zero = q == 0.0
                r0 = np.where(zero, 0.0, np.where(pos, c / q, q / a))
                r1 = np.where(zero, 0.0, np.where(pos, q / a, c / q))
                roots = [np.where(disc < 0.0, np.nan, r0), np.where(disc < 0.0, np.nan, r1)]
            for r, lam in enumerate(roots):
                adm = (lam >= -1e-12) & (lam <= 1.0 + 1e-12)
                lam = np.minimum(np.maximum(lam, 0.0), 1.0)
                tx, ty = t0x + lam * dtx, t0y + lam * dty
                fx, fy = ref[k, 0] + lam * ex, ref[k, 1] + lam * ey
                dd = (-(x - fx) * ty + (y - fy) * tx) / np.sqrt(tx * tx + ty * ty)
                cand = adm & (np.abs(dd) <= d_limit)
                sk = ref_pos[k] + lam * (ref_pos[k + 1] - ref_pos[k])
                if keep_candidates:
                    cand_ad[2 * k + r] = np.where(cand, np.abs(dd), np.nan)
                    cand_s[2 * k + r] = np.where(cand, sk, np.nan)
                take = cand & ((seg < 0) | (np.abs(dd) < np.abs(d)))
                s, d, lam_out, seg = np.where(take, sk, s), np.where(take, dd, d), np.where(take, lam, lam_out), np.where(take, k, seg)
    out = (s.reshape(shape), d.reshape(shape), seg.reshape(shape), lam_out.reshape(shape))
    return out + (cand_ad, cand_s) if keep_candidates else out


def near_ties(ref, ref_pos, x, y, d_limit=20.0):
    """Points with a second admissible candidate within 1e-6 m in |d| of the chosen one at an s more than 1e-6 m away: there the
    choice would hang on the last bit."""
    s, d, seg, _, cand_ad, cand_s = project_batch(ref, ref_pos, x, y, d_limit, keep_candidates=True)
    with np.errstate(invalid="ignore"):
        rival = (cand_ad - np.abs(d).ravel()[None] <= 1e-6) & (np.abs(cand_s - s.ravel()[None]) > 1e-6)
    return int(rival.any(axis=0).sum())


def valid_orientation(a):
    """make_valid_orientation, elementwise: into [-pi, pi)"""
    m = np.asarray(a, float) % TWO_PI
    return np.where((np.pi <= m) & (m <= TWO_PI), m - TWO_PI, m)


def curvilinear(ref, ref_pos, ref_theta, x, y, theta, d_limit=20.0):
    """(s, d, theta_cl) of poses; NaN outside the projection domain"""
    s, d, seg, lam = project_batch(ref, ref_pos, x, y, d_limit)
    k = np.maximum(seg, 0)
    ref_theta = np.asarray(ref_theta, float)
    with np.errstate(invalid="ignore"):
        th = valid_orientation(np.asarray(theta, float) - (ref_theta[k] + lam * (ref_theta[k + 1] - ref_theta[k])))
    return s, d, np.where(seg >= 0, th, np.nan)


# ---- ReactivePlanner._check_constraints, reactive_planner.py:971-1017 ------------------------------------------------------------
CHECK = {"velocity": 1, "acceleration": 2, "kappa": 4, "kappa_dot": 8, "yaw_rate": 16}
REASON = {"velocity": 1, "acceleration": 2, "kappa": 3, "kappa_dot": 4, "yaw_rate": 5}
OUT_OF_DOMAIN = 6


def check_constraints(p, v, kappa_gl, theta_gl, a, i):
    """0, or the reason code of the first failing check at step i"""
    mask, dt = int(p.constraint_mask), float(p.dt)
    if mask & CHECK["velocity"]:
        if v[i] < -EPS:
            return REASON["velocity"]
    kappa_max = np.tan(p.delta_max) / p.wheelbase
    if mask & CHECK["kappa"]:
        if abs(kappa_gl[i]) > kappa_max:
            return REASON["kappa"]
    if mask & CHECK["yaw_rate"]:
        yaw_rate = (theta_gl[i] - theta_gl[i - 1]) / dt if i > 0 else 0.
        theta_dot_max = kappa_max * v[i]
        if abs(round(yaw_rate, 5)) > theta_dot_max:
            return REASON["yaw_rate"]
    if mask & CHECK["kappa_dot"]:
        steering_angle = np.arctan2(p.wheelbase * kappa_gl[i], 1.0)
        kappa_dot_max = p.v_delta_max / (p.wheelbase * math.cos(steering_angle) ** 2)
        kappa_dot = (kappa_gl[i] - kappa_gl[i - 1]) / dt if i > 0 else 0.
        if abs(kappa_dot) > kappa_dot_max:
            return REASON["kappa_dot"]
    if mask & CHECK["acceleration"]:
        v_switch = p.v_switch
        a_max = p.a_max * v_switch / v[i] if v[i] > v_switch else p.a_max
        a_min = -p.a_max
        if not a_min <= a[i] <= a_max:
            return REASON["acceleration"]
    return 0


def kinematic_verdict(p, v, kappa, theta, a, L):
    """(reason, step) of the first failing step of poses 0 .. L - 1, (0, 0) if none; an array that is None reads as zeros"""
    zeros = np.zeros(L)
    v, kappa, a = (zeros if q is None else q for q in (v, kappa, a))
    for i in range(L):
        r = check_constraints(p, v, kappa, theta, a, i)
        if r:
            return r, i
    return 0, 0


# ---- DefaultCostFunction / DefaultCostFunctionFailSafe, cost_function.py:51-71, 82-92 ----------------------------------------
def cost_of(cost, a, v, s, d, theta_cl):
    if int(cost.kind) == 1:
        costs = np.sum((1 * a) ** 2)
        costs += np.sum((0.25 * d) ** 2) + (20 * d[-1]) ** 2
        costs += np.sum((0.25 * np.abs(theta_cl)) ** 2) + (5 * (np.abs(theta_cl[-1]))) ** 2
        return float(costs)
    costs = 0.0
    costs += np.sum((cost.w_a * a) ** 2)
    if not math.isnan(cost.desired_speed):
        costs += np.sum((5 * (v - cost.desired_speed)) ** 2) + (50 * (v[-1] - cost.desired_speed) ** 2) + \
                 (100 * (v[int(len(v) / 2)] - cost.desired_speed) ** 2)
    if not math.isnan(cost.desired_s):
        costs += np.sum((0.25 * (cost.desired_s - s)) ** 2) + (20 * (cost.desired_s - s[-1])) ** 2
    costs += np.sum((0.25 * (cost.desired_d - d)) ** 2) + (20 * (cost.desired_d - d[-1])) ** 2
    costs += np.sum((0.25 * np.abs(theta_cl)) ** 2) + (5 * (np.abs(theta_cl[-1]))) ** 2
    return float(costs)


# ---- the whole call ----------------------------------------------------------------------------------------------------------
def reference(p, cost, ref, ref_pos, ref_theta, x, y, theta, v=None, a=None, kappa=None, lengths=None, d_limit=20.0):
    """What rp_score_evaluate returns, as a namespace: s, d, theta_cl [K, n] (NaN outside the domain and behind the end), status [K]
    uint32, cost [K], best, best_cost, n_feasible, reason_counts [8]."""
    x, y, theta = (np.atleast_2d(np.asarray(q, float)) for q in (x, y, theta))
    v, a, kappa = (None if q is None else np.atleast_2d(np.asarray(q, float)) for q in (v, a, kappa))
    K, n = x.shape
    lengths = np.full(K, n) if lengths is None else np.asarray(lengths)
    valid = np.arange(n)[None, :] < lengths[:, None]
    s, d, th = curvilinear(ref, ref_pos, ref_theta, x, y, theta, d_limit)
    s, d, th = np.where(valid, s, np.nan), np.where(valid, d, np.nan), np.where(valid, th, np.nan)
    status, costs, counts = np.zeros(K, np.uint32), np.full(K, np.nan), np.zeros(8, np.int64)
    for k in range(K):
        L = int(lengths[k])
        row = lambda q: None if q is None else q[k, :L]   # noqa: E731
        reason, step = kinematic_verdict(p, row(v), row(kappa), theta[k, :L], row(a), L)
        if not reason:
            outside = np.flatnonzero(np.isnan(s[k, :L]))
            if outside.size:
                reason, step = OUT_OF_DOMAIN, int(outside[0])
        if reason:
            status[k] = 2 | (reason << 4) | (min(step, 0xFFF) << 8)
            counts[reason] += 1
        else:
            status[k] = 1
            costs[k] = cost_of(cost, row(a), row(v), s[k, :L], d[k, :L], th[k, :L])
    feasible = np.flatnonzero(status == 1)
    best = -1
    for k in feasible:   # lexicographic minimum of (cost, k); a NaN cost never wins
        if costs[k] == costs[k] and (best < 0 or costs[k] < costs[best]):
            best = int(k)
    return NS(s=s, d=d, theta_cl=th, status=status, cost=costs, best=best, best_cost=costs[best] if best >= 0 else math.nan,
              n_feasible=int(feasible.size), reason_counts=counts, valid=valid)


# ---- the draw fixtures -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(name):
    """A draw fixture as a namespace: the path's tables, params and cost, the stored blocks' rows and own lengths, and what the
    fixture says about them (reason, cost, label by block)."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    veh = z["vehicle"]
    p = make_params(dt=float(z["dt"]), N=int(z["N"]), factor=int(z["factor"]), time_step0=int(z["time_step0"]), low_vel_mode=bool(z["low_vel_mode"]),
                    lon_mode=int(z["lon_mode"]), constraint_mask=int(z["constraint_mask"]), x0_lon=z["x0_lon"], x0_lat=z["x0_lat"],
                    x0_orientation=float(z["x0_orientation"]), wheelbase=veh[0], wb_rear_axle=veh[1], length=veh[2], width=veh[3], a_max=veh[4],
                    v_switch=veh[5], delta_max=veh[6], v_delta_max=veh[7])
    ds, dss = float(z["desired_speed"]), float(z["desired_s"])
    cost = make_cost(kind=int(z["cost_kind"]), w_a=float(z["w_a"]), desired_speed=None if np.isnan(ds) else ds, desired_d=float(z["desired_d"]),
                     desired_s=None if np.isnan(dss) else dss)
    idx = z["state_index"]
    f = NS(name=name, p=p, cost=cost, ref=z["ref_path"], ref_pos=z["ref_pos"], ref_theta=z["ref_theta"], d_limit=float(z["proj_d_limit"]),
           states=z["states"], index=idx, lengths=z["traj_len"][idx // (len(z["L"]) * len(z["D"]))].astype(np.int32), n=int(z["N"]) + 1,
           reason=z["reason"][idx].astype(int), label=z["label"][idx].astype(int), fixture_cost=z["cost"][idx])
    for q in (f.ref, f.ref_pos, f.ref_theta, f.states, f.lengths):
        q.setflags(write=False)
    return f


def fixture_rows(f):
    st = f.states
    return dict(x=st[:, RP_X], y=st[:, RP_Y], theta=st[:, RP_THETA], v=st[:, RP_V], a=st[:, RP_A], kappa=st[:, RP_KAPPA], lengths=f.lengths)


@functools.lru_cache(maxsize=None)
def fixture_reference(name):
    """The reference's answer on a fixture's stored blocks, each over its OWN length (see tests/test_score_abi.py for why)."""
    f = fixture(name)
    return reference(f.p, f.cost, f.ref, f.ref_pos, f.ref_theta, d_limit=f.d_limit, **fixture_rows(f))


# ---- shapes where the mapping can go wrong ---------------------------------------------------------------------------------------
# (name, K, n_poses, ragged lengths, path, largest lateral offset [m]): trajectories with lateral offsets up to 3 m on paths whose
# curvature radius stays above 6 m; the last two keep 12 to 16 m from a path of 0.5 m segments (curvature radius >= 40 m), where a pose
# has more open segments than a lane lists for itself and the wavefront falls back to the plain walk
SHAPES = [
    ("one_pose", 3, 1, False, "cfg2", 3.0),
    ("n63", 1, 63, False, "cfg2", 3.0),
    ("n64_ragged", 3, 64, True, "cfg2", 3.0),
    ("n65_k257", 257, 65, True, "cfg1", 3.0),
    ("n130", 3, 130, True, "cfg2", 3.0),
    ("one_segment", 3, 65, True, "two_vertex", 3.0),
    ("lds_cap", 3, 63, True, "at_cap", 3.0),
    ("lds_cap_plus_one", 3, 63, True, "beyond_cap", 3.0),
    ("far_lds", 5, 65, True, "at_cap", 16.0),
    ("far_device_memory", 5, 65, True, "beyond_cap", 16.0),
]
SEED = 2025


def long_path(n_seg):
    """A gentle S of n_seg segments of 0.5 m, curvature radius >= 40 m: the tables of frontend.build_reference without smoothing."""
    sarc = 0.5 * np.arange(n_seg + 1)
    heading = 0.6 * np.sin(sarc / 40.0)   # |d heading / ds| <= 0.015 / m
    pts = np.concatenate(([[0.0, 0.0]], np.cumsum(0.5 * np.stack((np.cos(heading[:-1]), np.sin(heading[:-1])), 1), axis=0)))
    ref, pos, th, _, _ = frontend.build_reference(pts, smooth=False)
    assert len(ref) == n_seg + 1
    return ref, pos, th


@functools.lru_cache(maxsize=None)
def path(kind):
    if kind in ("cfg1", "cfg2"):
        f = fixture("cfg1_ref_l1_draw" if kind == "cfg1" else "cfg2_ref_draw")
        return f.ref, f.ref_pos, f.ref_theta
    if kind == "two_vertex":
        ref, pos, th, _, _ = frontend.build_reference(np.array([[3.0, -2.0], [83.0, 38.0]]), smooth=False)
        return ref, pos, th
    if kind == "u":
        ref, pos, th, _, _ = frontend.build_reference(U_PATH, smooth=False)
        return ref, pos, th
    return long_path(LDS_ROWS if kind == "at_cap" else LDS_ROWS + 1)


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """Inputs of one shape and the reference's answer.  A trajectory is drawn in the path's frame -- s advancing with a noisy speed, d
    within 3 m of the path -- and mapped to Cartesian poses by the definition the projection inverts (foot point + d * normal of the
    interpolated vertex tangent); its heading is the path's plus noise, and v, a, kappa carry noise and a few spikes so that every
    check fails somewhere and most trajectories pass."""
    _, K, n, ragged, kind, lateral = next(c for c in SHAPES if c[0] == name)
    rng = np.random.default_rng([SEED, [c[0] for c in SHAPES].index(name)])
    ref, pos, th_ref = path(kind)
    f = fixture("cfg2_ref_draw")
    total, dt = pos[-1], 0.1
    v0 = rng.uniform(0.2, min(8.0, 0.45 * total / (n * dt)), (K, 1))
    acc = rng.normal(0.0, 1.0, (K, n))
    v = v0 + np.cumsum(acc, 1) * dt
    s = rng.uniform(0.05 * total, 0.4 * total, (K, 1)) + np.cumsum(np.maximum(v, 0.0), 1) * dt
    side = rng.uniform(-2.7, 2.7, (K, 1)) if lateral <= 3.0 else rng.choice([-1.0, 1.0], (K, 1)) * rng.uniform(12.3, lateral - 0.3, (K, 1))
    d = side + 0.3 * np.sin(rng.uniform(0.0, 6.0, (K, 1)) + 0.2 * np.arange(n)[None, :])
    k0 = np.clip(np.searchsorted(pos, s, side="right") - 1, 0, len(pos) - 2)
    lam = (s - pos[k0]) / (pos[k0 + 1] - pos[k0])
    tan = frontend.compute_vertex_tangents(ref)
    foot = ref[k0] + lam[..., None] * (ref[k0 + 1] - ref[k0])
    t = tan[k0] + lam[..., None] * (tan[k0 + 1] - tan[k0])
    t = t / np.sqrt((t * t).sum(-1))[..., None]
    x, y = foot[..., 0] - d * t[..., 1], foot[..., 1] + d * t[..., 0]
    theta = th_ref[k0] + lam * (th_ref[k0 + 1] - th_ref[k0]) + rng.normal(0.0, 0.004, (K, n))
    kappa = rng.normal(0.0, 0.02, (K, 1)) + np.cumsum(rng.normal(0.0, 0.004, (K, n)), 1)
    for q in range(0, K, 7):   # a spike each in a, kappa and theta of some trajectories, at a random step
        j = int(rng.integers(0, n))
        which = (q // 7) % 4
        if which == 0:
            acc[q, j] = 15.0
        elif which == 1:
            kappa[q, j:] += 1.0
        elif which == 3:
            kappa[q, j:] += 0.05
        else:
            theta[q, j:] += 0.6
    lengths = None
    if ragged:
        lengths = rng.integers(1, n + 1, K).astype(np.int32)
        lengths[0], lengths[-1] = n, 1
    c = NS(name=name, p=f.p, cost=f.cost, ref=ref, ref_pos=pos, ref_theta=th_ref, d_limit=20.0, x=x, y=y, theta=theta, v=v, a=acc, kappa=kappa,
           lengths=lengths, lateral=lateral)
    c.ref_out = reference(c.p, c.cost, ref, pos, th_ref, x, y, theta, v, acc, kappa, lengths)
    for q in (x, y, theta, v, acc, kappa):
        q.setflags(write=False)
    return c


def case_rows(c):
    return dict(x=c.x, y=c.y, theta=c.theta, v=c.v, a=c.a, kappa=c.kappa, lengths=c.lengths)


def status_word(label, reason=0, step=0):
    return label | (reason << 4) | (step << 8)
