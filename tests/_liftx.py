"""The lifted state planes against the extended-precision reference (TEST INFRASTRUCTURE: tests/test_liftx_abi.py on the CPU,
tests/test_liftx.py on the GPU).  What librp_lift computes from six given curvilinear planes -- x, y, theta, v, a, kappa, kappa_dot,
theta_cl -- and what librp_pick and librp_epick, which compile the same walk, compute and cost, held to ``_xref.per_pose``: the
reference planner's per-pose formulas in double-word ``longdouble`` arithmetic (tests/_dd.py) on the DOUBLE inputs, rounded on output.
No horizon extension: the lift has none.  The cost is include/rp_pick.h's, over a trajectory's own len[k] poses (last entry pose
len[k] - 1, middle entry v[len[k] / 2]), summed in double-word arithmetic from the double-word rows and the given s, d.

The comparison is ``_xref``'s rule with ``_xref``'s constants and takes no number from the device.  With X the reference,
O = ``_lift.reference`` (double) and D a device result, per case and plane over the compared poses -- those where O holds a number;
the NaN pattern, status words and reductions stay with tests/test_lift.py, test_pick.py and test_epick.py --

    E_D <= 8 E_O + 8 spacing(scale)        R_D <= 4 R_O + 2 spacing(scale)

and for the cost of a kinematically feasible trajectory of len poses, relative: 8 x the oracle's worst + _bitid.summation_bound(len),
the oracle's cost being ``_score.cost_of`` on O's planes.  A trajectory whose O is further than ``_xref.LEFT_OUT_ABOVE`` from X on a
compared pose is left out: decided from O and X alone.

The cases:
  lift:*      every case of ``_lift.CASES`` with its own path and params (what each exercises: tests/test_lift.py)
  fixture:*   the four ``_lift.GPU_FIXTURES``
  xref:*      the candidates' planes (``_kin_plan.lift_planes``) of ``_xref`` cases on the case's own path; desired_d up to 4 m on the
              25 m arc makes 1 - k_r d do real work
  wrapped            8 x 80 on ``_xref``'s 25 m arc, s within 43 .. 140 m: the unwrapped table heading passes pi (at s = 68.5 m) and stays
                     beyond it, make_valid_orientation does the work.  Trajectory 4 crosses the wrap between poses 63 and 64 (two chunks of
                     the walk), trajectory 5 between poses 20 and 21.  |d| <= 0.008 m and |d'| <= 1e-3, so that a float32 reciprocal, atan
                     or tangent length moves a pose by less than the 1e-9 of the earlier contract (tests/test_liftx_abi.py plants them).
                     Condition: every compared pose's table heading is at least 1e-6 rad from an odd multiple of pi.
  three_chunks_130   3 x 130 on ``_xref``'s S-curve: standstills from pose 126, 127 (lane 63 of the second chunk) and 128 (lane 0 of
                     the third) to the end; the second row ends on pose 128, the others on 129
  three_chunks_193   2 x 193, standstills over poses 126 .. 130 and 191 .. 192: theta, kappa and the kept orientation are carried into a
                     third and a fourth chunk
  tight_hv, tight_lv 8 x 40 each on a 6 m arc, d toward the centre from 0 to 5 m (1 - k_r d from 1 down to 1/6) and 2.5 and 5 m outside.
                     NARROWED: the arc has the shape and rotation of ``_proj``'s arc6 but starts at (3e3, -2.1e3), not (3e6, -2.1e6).
                     At 3e6 half a spacing of a coordinate is 2.3e-10 m: every trajectory's O would be beyond LEFT_OUT_ABOVE = 1e-10
                     and E_O beyond ORACLE_BOUND = 1e-11, which this module does not raise.  So x and y at a scale of 3e6, where the
                     rule's floor would follow the scale, are NOT held by this rule (the six other planes never read the vertices).
  steep_lv           8 x 20, low-velocity mode on the 25 m arc, d' = 0, 0.5, 2, 6, 14 and -2, -6, -14 (theta_cl up to 1.4995 rad)
  steep_hv           8 x 12, s_dot from 0.001 (1 + 1.25e-9) to 0.01 and one at 0.001 (1 - 1.25e-9), which stands still and keeps its
                     theta0; d_dot up to 0.01 (d' up to 10).  (1.25e-9: the double next to 0.001 (1 + 1e-9) is 4e-18 short of 1e-9.)
                     Condition: every s_dot is at least 1e-9 relative from 0.001 and from 1e-5, on the side its row intends.
The new families run with constraint_mask = 0: every trajectory is kinematically feasible and has a cost.

usage: python tests/_liftx.py [out_file]      writes profiles/accuracy_lift.txt (the device's columns where there is a GPU)"""
import functools
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

if __name__ == "__main__":   # (as a script: the paths tests/conftest.py sets up for the suite)
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "commonroad-reactive-planner_amd"), os.path.join(_repo, "tests")]

import _dd as dd
import _lift as L
import _score as S
import _xref as X
from _bitid import summation_bound
from _dd import DD
from commonroad_rp_amd._capi import RpError, RpLibraryMissing, RpParams, make_cost, COST_DEFAULT, COST_FAILSAFE
from oracle import frontend

LD = X.LD
PLANES = L.PLANES
ROWS14 = (X.X, X.Y, X.THETA, X.V, X.A, X.KAPPA, X.KAPPA_DOT, X.THETA_CL)   # rows of ``_xref.per_pose`` the eight planes are
CHUNK = 64                      # poses a wavefront of the walk takes at a time
LDS_ROWS = L.LDS_ROWS
LEFT_OUT_CAP_NEW = 0.02         # of a new family's trajectories: the cap ``_xref`` gives its degenerate cases
WRAP_CLEAR = 1e-6               # rad, distance of a table heading from an odd multiple of pi
RULE_CLEAR = 1e-9               # relative distance of s_dot from 0.001 and 1e-5


# ---- the reference -------------------------------------------------------------------------------------------------------------
def tables_of(t):
    """a path namespace of ``_lift`` (ref, pos, theta, curv, curv_d) as the tables ``_xref.per_pose`` reads"""
    return NS(ref_pos=t.pos, ref_theta=t.theta, ref_curv=t.curv, ref_curv_d=t.curv_d, ref_x=np.ascontiguousarray(t.ref[:, 0]),
              ref_y=np.ascontiguousarray(t.ref[:, 1]))


def cost_own_length(c, st, tl):
    """include/rp_pick.h: cost_function.py:51-71 (default), :82-92 (fail-safe) over each trajectory's own tl poses -- the last entry is
    pose tl - 1, the middle entry v[tl / 2] --, plain sums in order, double-word, from the rows of ``_xref.per_pose``"""
    a, v, s, d, th = (st[r] for r in (X.A, X.V, X.S, X.D, X.THETA_CL))
    m, n = a.shape
    valid = np.arange(n)[None, :] < tl[:, None]
    rows, last, mid = np.arange(m), tl - 1, tl // 2

    def total(term):
        w = dd.where(valid, term, 0)
        return dd.total(w, n, lambda i: w[:, i])
    at = lambda row, i: row[rows, i]
    q = LD(0.25)
    tail = total((q * abs(th)) ** 2) + (5 * abs(at(th, last))) ** 2
    if c.kind == COST_FAILSAFE:
        return total(a * a) + total((q * d) ** 2) + (20 * at(d, last)) ** 2 + tail
    cost = total((LD(c.w_a) * a) ** 2)
    if not math.isnan(c.desired_speed):
        vd = LD(c.desired_speed)
        cost = cost + total((5 * (v - vd)) ** 2) + (50 * (at(v, last) - vd) ** 2) + (100 * (at(v, mid) - vd) ** 2)
    if not math.isnan(c.desired_s):
        ds = LD(c.desired_s)
        cost = cost + total((q * (ds - s)) ** 2) + (20 * (ds - at(s, last))) ** 2
    dsd = LD(c.desired_d)
    cost = cost + total((q * (dsd - d)) ** 2) + (20 * (dsd - at(d, last))) ** 2
    return cost + tail


def evaluate(p, t, planes, lengths=None, theta0=None, costs=()):
    """The reference of one lift call: params, a path namespace, the six double planes [K, n], lengths and theta0 as rp_lift_evaluate
    takes them -> namespace(rows [K, 8, n] longdouble in the order of ``PLANES``, cost: one [K] longdouble per rp_cost of ``costs``,
    inter: the intermediates of ``_xref.per_pose``).  Poses behind a length are zero, poses off the path whatever the formulas give:
    the comparison reads neither."""
    planes = [np.atleast_2d(np.asarray(q, np.float64)) for q in planes]
    K, n = planes[0].shape
    tl = np.full(K, n, np.int64) if lengths is None else np.asarray(lengths).astype(np.int64)
    valid = np.arange(n)[None, :] < tl[:, None]
    th0 = LD(p.x0_orientation) if theta0 is None else np.asarray(theta0, np.float64).astype(LD)
    with np.errstate(all="ignore"):   # (off-path and NaN poses: masked by the comparison)
        st, inter = X.per_pose(bool(p.low_vel_mode), tables_of(t), *(dd.where(valid, X._dd_in(q), 0) for q in planes), valid, th0)
        rows = np.stack([st[r].ld() for r in ROWS14], axis=1)
        cost = [cost_own_length(c, st, tl).ld() for c in costs]
    inter = {k: v.ld() for k, v in inter.items()}
    X._readonly(rows, *cost, *inter.values())
    return NS(rows=rows, cost=cost, inter=inter, lengths=tl)


def stacked(o):
    """the eight planes of a lift result (``_lift.reference``'s namespace or the device's) as [K, 8, n]"""
    return np.stack([np.asarray(getattr(o, name), np.float64) for name in PLANES], axis=1)


def oracle_cost(cost, o, planes):
    """[K]: ``_score.cost_of`` on O's planes and the given s, d; NaN where O is not kinematically feasible"""
    out = np.full(len(o.status), np.nan)
    for k in np.flatnonzero(o.status == 1):
        m = int(o.lengths[k])
        out[k] = S.cost_of(cost, o.a[k, :m], o.v[k, :m], planes[0][k, :m], planes[3][k, :m], o.theta_cl[k, :m])
    return out


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def compare_planes(Xs, O, Dv):
    """``_xref``'s rule per plane: Xs [K, 8, n] longdouble, O and Dv [K, 8, n] doubles.  Compared: where O holds a number, per plane.
    -> (eight ``_xref.RowResult``, number of trajectories left out, which [K]).  A device value that is no number on a compared pose
    exceeds every bound."""
    mask = np.isfinite(O)
    with np.errstate(invalid="ignore"):
        dev_o = np.abs(np.asarray(O).astype(LD) - Xs)
        out = ((~(dev_o <= X.LEFT_OUT_ABOVE)) & mask).any(axis=(1, 2))
        dev_d = np.abs(np.where(np.isfinite(Dv), Dv, np.inf).astype(LD) - Xs)
    sel = mask & ~out[:, None, None]
    rows = []
    for r, name in enumerate(PLANES):
        q = sel[:, r, :]
        cnt = max(int(q.sum()), 1)
        eo, ed = np.where(q, dev_o[:, r], LD(0)), np.where(q, dev_d[:, r], LD(0))
        scale = float(np.where(q, np.abs(Xs[:, r]), LD(0)).max())
        sp = float(np.spacing(scale))
        e_o, e_d = float(eo.max()), float(ed.max())
        r_o, r_d = float(np.sqrt((eo * eo).sum() / cnt)), float(np.sqrt((ed * ed).sum() / cnt))
        rows.append(X.RowResult(name, scale, e_o, e_d, r_o, r_d, X.MARGIN_MAX * e_o + X.FLOOR_MAX * sp, X.MARGIN_RMS * r_o + X.FLOOR_RMS * sp))
    return rows, int(out.sum()), out


def compare_costs(cX, cO, cD, sel, lengths):
    """costs of the trajectories sel [K] (kinematically feasible in O, not left out), relative to the reference's
    -> (the oracle's worst, the device's worst, the bound of the device's worst trajectory, every trajectory within its bound)"""
    idx = np.flatnonzero(sel)
    if not idx.size:
        return 0.0, 0.0, 0.0, True
    cx = cX[idx]
    rel = lambda c: (np.abs(np.asarray(c)[idx].astype(LD) - cx) / cx).astype(np.float64)
    with np.errstate(invalid="ignore"):
        rel_o, rel_d = rel(cO), rel(np.where(np.isfinite(cD), cD, np.inf))
    e_o = float(rel_o.max())
    bound = X.MARGIN_MAX * e_o + np.array([summation_bound(int(n)) for n in np.asarray(lengths)[idx]])
    worst = int(np.argmax(rel_d - bound))
    return e_o, float(rel_d.max()), float(bound[worst]), bool((rel_d <= bound).all())


# ---- the cases -------------------------------------------------------------------------------------------------------------------
XREF_CASES = X.CASE_NAMES
NEW_FAMILIES = ("wrapped", "three_chunks_130", "three_chunks_193", "tight_hv", "tight_lv", "steep_lv", "steep_hv")
CASE_NAMES = tuple("lift:" + n for n in L.CASES) + tuple("fixture:" + n for n in L.GPU_FIXTURES) + tuple("xref:" + n for n in XREF_CASES) + NEW_FAMILIES
COST_CASES = tuple(n for n in CASE_NAMES if not n.startswith(("lift:", "fixture:")))   # rp_pick_select and rp_epick_select run these
SEED = 2028
# the cases that run on both table variants (``fits_both``; tests/test_liftx_abi.py holds this list to it)
BOTH_VARIANTS = tuple("lift:" + n for n in ("one_pose", "n63", "n64", "n65", "n129", "ragged", "standstill_head", "standstill_head_theta0", "standstill_across",
                                            "standstill_all", "stop_and_go", "low_vel", "off_start", "beyond_d", "nan_input", "many")) + \
    tuple("fixture:" + n for n in L.GPU_FIXTURES) + tuple("xref:" + n for n in ("arc_keep_n17", "arc_low_n65", "arc_failsafe_n64", "arc_draw_n17", "arc_draw_stop_n16")) + \
    ("wrapped", "tight_hv", "tight_lv", "steep_lv", "steep_hv")


def family(name):
    return "a" if name.startswith(("lift:", "fixture:")) else "b" if name.startswith("xref:") else "c"


def _own_params(p, **changes):
    q = RpParams.from_buffer_copy(p)
    for k, v in changes.items():
        setattr(q, k, v)
    return q


def xref_path(name):
    """the path of an ``_xref`` case as a path namespace of ``_lift``"""
    co = X.case(name).co
    return NS(ref=co.reference, pos=co.ref_pos, theta=co.ref_theta, curv=co.ref_curv, curv_d=co.ref_curv_d, d_limit=float(co.proj_domain_d_limit),
              tan=frontend.compute_vertex_tangents(co.reference))


def _along(t, n, s0, v0, d0, amp, q, phi, low):
    """s = s0 + v0 t; d = d0 + amp sin(q (s - s0) + phi) along the path with its exact derivatives: d', d'' in low-velocity mode,
    d_dot = d' s_dot and d_ddot = d'' s_dot^2 otherwise"""
    s0, v0, d0, amp, q, phi = (np.asarray(a, float).reshape(-1, 1) for a in np.broadcast_arrays(s0, v0, d0, amp, q, phi))
    tt = L.DT * np.arange(n)[None, :]
    s, sd = s0 + v0 * tt, v0 + 0.0 * tt
    arg = q * (s - s0) + phi
    d, g1, g2 = d0 + amp * np.sin(arg), amp * q * np.cos(arg), -amp * q * q * np.sin(arg)
    return [s, sd, 0.0 * tt * v0, d, g1, g2] if low else [s, sd, 0.0 * tt * v0, d, g1 * sd, g2 * sd * sd]


def wrap_point(t):
    """the arc length at which the unwrapped table heading passes pi (the first one)"""
    k = int(np.flatnonzero((t.theta[:-1] < math.pi) & (t.theta[1:] >= math.pi))[0])
    return float(t.pos[k] + (math.pi - t.theta[k]) / (t.theta[k + 1] - t.theta[k]) * (t.pos[k + 1] - t.pos[k]))


def _tight_path():
    """a 6 m arc of three quarters of a turn in 0.25 m segments, turned by 0.7 rad, from (3e3, -2.1e3)"""
    radius, sweep = 6.0, 1.5 * np.pi
    ang = np.linspace(0.0, sweep, int(round(radius * sweep / 0.25)) + 1)
    c, sn = math.cos(0.7), math.sin(0.7)
    pts = np.stack((radius * np.sin(ang), radius * (1.0 - np.cos(ang))), 1) @ np.array([[c, sn], [-sn, c]]) + np.array([3.0e3, -2.1e3])
    return L.built_path(pts)


def _new_family(name):
    f = S.fixture("cfg2_ref_draw")
    p, lengths, theta0 = _own_params(f.p, constraint_mask=0), None, None
    if name == "wrapped":
        t = xref_path("arc_keep_n17")
        sw, n = wrap_point(t), 80
        v0 = np.array([5.0, 5.0, 5.0, 5.0, 4.0, 6.0, 2.0, 3.0])
        s0 = np.array([70.0, 80.0, 90.0, 100.0, sw - 4.0 * L.DT * 63.5, sw - 6.0 * L.DT * 20.5, 71.0, 110.0])
        planes = _along(t, n, s0, v0, [0.004, -0.004, 0.0, 0.002, -0.002, 0.004, 0.0, -0.004], 0.004, 0.2, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 0.5, 1.5], False)
    elif name.startswith("three_chunks"):
        t = xref_path("scurve_stop_n64")
        n = int(name[-3:])
        stops = {130: ([(126, 129)], [(127, 129)], [(128, 129)]), 193: ([(126, 130), (191, 192)], [(127, 131), (191, 192)])}[n]
        total = t.pos[-1] - t.pos[0]
        rows = [L._speed_profile(np.random.default_rng([SEED, n, k]), 1, n, total, st) for k, st in enumerate(stops)]
        planes = [np.concatenate([r[q] for r in rows], axis=0) for q in range(6)]
        lengths = np.array([130, 129, 130], np.int32) if n == 130 else None
    elif name.startswith("tight"):
        t = _tight_path()
        low = name.endswith("lv")
        p = _own_params(p, low_vel_mode=int(low))
        d0 = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.95, -2.5, -4.95])
        planes = _along(t, 40, 3.0 + np.arange(8.0), 3.0, d0, 0.05, 0.8, np.arange(8.0), low)
    elif name == "steep_lv":
        t = xref_path("arc_keep_n17")
        p = _own_params(p, low_vel_mode=1)
        g1 = np.array([0.0, 0.5, 2.0, 6.0, 14.0, -2.0, -6.0, -14.0])[:, None]
        n = 20
        tt = L.DT * np.arange(n)[None, :]
        s = (20.0 + 10.0 * np.arange(8.0))[:, None] + 0.5 * tt
        d = 0.3 - 0.5 * g1 * 0.5 * (n - 1) * L.DT + g1 * (s - s[:, :1])
        planes = [s, np.full((8, n), 0.5), np.zeros((8, n)), d, g1 + 0.0 * tt, np.full((8, n), 0.01)]
    elif name == "steep_hv":
        t = xref_path("arc_keep_n17")
        sd = np.array([0.001 * (1 + 1.25e-9), 0.001 * (1 + 1e-6), 0.002, 0.005, 0.01, 0.001 * (1 - 1.25e-9), 0.01, 0.003])[:, None]
        d_dot = np.array([0.01, 0.005, 0.01, -0.01, 0.01, 0.01, 0.0, -0.004])[:, None]
        n = 12
        tt = L.DT * np.arange(n)[None, :]
        s = (30.0 + 9.3 * np.arange(8.0))[:, None] + sd * tt
        d = np.linspace(-1.5, 1.5, 8)[:, None] + d_dot * tt
        planes = [s, sd + 0.0 * tt, np.zeros((8, n)), d, d_dot + 0.0 * tt, np.full((8, n), 1e-6)]
        theta0 = np.linspace(-0.5, 3.0, 8)
    else:
        raise KeyError(name)
    return p, t, planes, lengths, theta0, (f.cost, make_cost(COST_FAILSAFE))


@functools.lru_cache(maxsize=None)
def case(name):
    """One case, read-only: namespace(name, family, p, path, planes (six [K, n]), lengths, theta0, costs (the rp_cost structs the picks
    are called with: a default and a fail-safe one; none in family a), out: O, the namespace of ``_lift.reference``)"""
    costs = ()
    if name.startswith("lift:"):
        c = L.case(name[5:])
        p, t, planes, lengths, theta0, o = c.p, c.path, c.planes, c.lengths, c.theta0, c.out
    elif name.startswith("fixture:"):
        q = L.fixture_inputs(name[8:])
        p, t, lengths, theta0 = S.fixture(name[8:]).p, L.fixture_path(name[8:]), q["lengths"], None
        planes = tuple(q[k] for k in ("s", "s_dot", "s_ddot", "d", "d_dot", "d_ddot"))
        o = L.fixture_reference(name[8:])
    elif name.startswith("xref:"):
        import _kin_plan
        c = X.case(name[5:])
        planes, lengths = _kin_plan.lift_planes(name[5:])
        p, t, theta0 = c.inp.params, xref_path(name[5:]), None
        own = c.inp.cost
        costs = (own, make_cost(COST_FAILSAFE)) if own.kind == COST_DEFAULT else (make_cost(COST_DEFAULT, w_a=1.0, desired_speed=8.0, desired_d=0.5), own)
        o = L.reference(p, t, *planes, lengths=lengths, theta0=theta0)
    else:
        p, t, planes, lengths, theta0, costs = _new_family(name)
        o = L.reference(p, t, *planes, lengths=lengths, theta0=theta0)
    planes = tuple(np.ascontiguousarray(np.atleast_2d(np.asarray(q, np.float64))) for q in planes)
    for q in planes:
        q.setflags(write=False)
    return NS(name=name, family=family(name), p=p, path=t, planes=planes, lengths=lengths, theta0=theta0, costs=costs, out=o)


@functools.lru_cache(maxsize=None)
def reference(name):
    """X of a case (``evaluate``), with the reference's cost per rp_cost of the case"""
    c = case(name)
    return evaluate(c.p, c.path, c.planes, c.lengths, c.theta0, c.costs)


@functools.lru_cache(maxsize=None)
def oracle_view(name):
    """(O as [K, 8, n], the oracle's costs: one [K] per rp_cost of the case), read-only"""
    c = case(name)
    return X._readonly(stacked(c.out), *(oracle_cost(k, c.out, c.planes) for k in c.costs))


def cpu_rows(name):
    """the comparison with O in the device's place: E_O, R_O, scale and the trajectories left out"""
    o = oracle_view(name)[0]
    return compare_planes(reference(name).rows, o, o)


def cost_selection(name):
    """[K] bool: kinematically feasible in O and not left out"""
    return (case(name).out.status == 1) & ~cpu_rows(name)[2]


# ---- the conditions of the new families, from the reference's intermediates ------------------------------------------------------
def compared_poses(name):
    """[K, n] bool: poses on which O holds theta"""
    return np.isfinite(case(name).out.theta)


def wrap_distance(name):
    """smallest distance of a compared pose's interpolated table heading from an odd multiple of pi"""
    th = reference(name).inter["th_table"][compared_poses(name)]
    k = np.rint((th / LD(math.pi) - 1) / 2)
    return float(np.abs(th - (2 * k + 1) * LD(math.pi)).min())


def wrap_crossings(name):
    """[(trajectory, pose i)]: the table heading of poses i - 1 and i lies on different sides of an odd multiple of pi"""
    th = reference(name).inter["th_table"]
    side = np.floor((th / LD(math.pi) + 1) / 2)
    ok = compared_poses(name)
    return [(int(k), int(i) + 1) for k, i in zip(*np.nonzero((side[:, 1:] != side[:, :-1]) & ok[:, 1:] & ok[:, :-1]))]


def rule_distance(name):
    """smallest relative distance of a compared pose's |s_dot| from 0.001 and from 1e-5, of its |d_dot| from 1e-5 (zeros apart)"""
    c, ok = case(name), compared_poses(name)
    sd, dv = np.abs(c.planes[1][ok].astype(LD)), np.abs(c.planes[4][ok].astype(LD))
    gaps = [np.abs(sd - X.S_VEL_MIN) / X.S_VEL_MIN, np.where(sd == 0, LD(1), np.abs(sd - X.EPS) / X.EPS), np.where(dv == 0, LD(1), np.abs(dv - X.EPS) / X.EPS)]
    return float(min(g.min() for g in gaps))


def standstill_starts(name):
    """[(trajectory, pose i)] of a high-velocity case: pose i stands still (s_dot <= 0.001 behind the 1e-5 rule) and keeps an orientation
    it did not compute -- pose i - 1 moved, or i = 0 and theta0 is read"""
    c = case(name)
    if c.p.low_vel_mode:
        return []
    sd = np.where(np.abs(c.planes[1]) < 1e-5, 0.0, c.planes[1])
    still = ~(sd > 0.001) & compared_poses(name)
    starts = still.copy()
    starts[:, 1:] &= ~still[:, :-1]
    return [(int(k), int(i)) for k, i in zip(*np.nonzero(starts))]


def coverage():
    """what the cases reach, from their inputs: lanes (pose index mod 64) on which a standstill's carry starts, wrap crossings inside a
    chunk and across a chunk boundary, segment counts on both sides of the LDS capacity"""
    lanes = {(i % CHUNK, i >= CHUNK) for name in CASE_NAMES for _, i in standstill_starts(name)}
    cross = wrap_crossings("wrapped")
    segs = {len(case(name).path.pos) - 1 for name in CASE_NAMES}
    return NS(carry_lane63=any(lane == CHUNK - 1 for lane, _ in lanes), carry_lane0_head=(0, False) in lanes, carry_lane0_across=(0, True) in lanes,
              wrap_inside=any(i % CHUNK for _, i in cross), wrap_across=any(i % CHUNK == 0 for _, i in cross),
              table_lds=any(q <= LDS_ROWS for q in segs), table_device_memory=any(q > LDS_ROWS for q in segs))


# ---- the same path with more rows ------------------------------------------------------------------------------------------------
TAIL = (100.0, 40.0, 10.0)   # tests/_proj.py's: straight on from the last vertex


def fits_both(name):
    """the case can run on both table variants with the SAME reference: its path has room for a tail below LDS_ROWS segments, and no
    pose reaches the last segment -- the one whose end tangent a tail changes"""
    c = case(name)
    s = c.planes[0][np.isfinite(c.planes[0])]
    return len(c.path.pos) - 1 < LDS_ROWS and bool((s < c.path.pos[-2]).all())


def padded(t, n_seg):
    """the path namespace filled up to n_seg segments by a straight tail: vertices straight on, heading kept, curvature 0"""
    extra = n_seg - (len(t.pos) - 1)
    assert extra >= 1
    e = t.ref[-1] - t.ref[-2]
    run = np.cumsum(np.resize(TAIL, extra))
    ref = np.concatenate((t.ref, t.ref[-1] + run[:, None] * (e / math.hypot(*e))))
    return NS(ref=ref, pos=np.concatenate((t.pos, t.pos[-1] + run)), theta=np.concatenate((t.theta, np.full(extra, t.theta[-1]))),
              curv=np.concatenate((t.curv, np.zeros(extra))), curv_d=np.concatenate((t.curv_d, np.zeros(extra))), d_limit=t.d_limit,
              tan=frontend.compute_vertex_tangents(ref))


# ---- a NumPy restatement of the lift in double, with the defects tests/test_liftx_abi.py plants -----------------------------------
DEFECTS = ("rcp_f32", "atan_f32", "lam_f32_curvature", "rsqrt_f32", "carry_f32", "cost_sums_f32")   # the last one: ``restated_cost``, on honest planes


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _fma(a, b, c):
    """a b + c rounded once (the product exact in double-word arithmetic)"""
    a, b, c = np.broadcast_arrays(a, b, c)
    return (DD(a.astype(LD)) * DD(b.astype(LD)) + DD(c.astype(LD))).ld().astype(np.float64)


def restate(p, t, planes, theta0=None, defect=None, contracted=False):
    """The lift's formulas on arrays, in double -> [K, 8, n] (no NaN pattern: the comparison reads O's).  ``defect``: one of DEFECTS.
    ``contracted``: products feeding a sum go through fma and the sums and products are associated the other way -- an honest variant."""
    assert defect is None or defect in DEFECTS
    s, sd, sdd, d, dv, da = (np.atleast_2d(np.asarray(q, np.float64)) for q in planes)
    K, n = s.shape
    fma = _fma if contracted else (lambda a, b, c: a * b + c)
    with np.errstate(all="ignore"):
        sd, dv = np.where(np.abs(sd) < S.EPS, 0.0, sd), np.where(np.abs(dv) < S.EPS, 0.0, dv)
        low = bool(p.low_vel_mode)
        moving = sd > 0.001
        if low:
            dp, dpp = dv, da
        else:
            rcp = 1.0 / np.where(moving, sd, 1.0)
            rcp = _f32(rcp) if defect == "rcp_f32" else rcp
            dp = np.where(moving, dv * rcp, 0.0)
            dpp = np.where(moving, fma(-dp, sdd, da) * (rcp * rcp) if contracted else (da - dp * sdd) * rcp * rcp, 0.0)
        k = np.clip(np.searchsorted(t.pos, s, side="right") - 1, 0, len(t.pos) - 2)
        seg = t.pos[k + 1] - t.pos[k]
        lam = (s - t.pos[k]) / seg
        th_ref = S.valid_orientation((t.theta[k + 1] - t.theta[k]) * (s - t.pos[k]) / seg + t.theta[k])
        theta_cl = np.arctan(dp.astype(np.float32)).astype(np.float64) if defect == "atan_f32" else np.arctan(dp)
        theta = theta_cl + th_ref
        use = moving | low
        th0 = np.full(K, float(p.x0_orientation)) if theta0 is None else np.asarray(theta0, float)
        for i in range(n):
            theta[:, i] = np.where(use[:, i], theta[:, i], th0 if i == 0 else theta[:, i - 1])
        theta_cl = np.where(use, theta_cl, theta - th_ref)
        lam_c = _f32(lam) if defect == "lam_f32_curvature" else lam
        k_r = fma(t.curv[k + 1] - t.curv[k], lam_c, t.curv[k])
        k_r_d = fma(t.curv_d[k + 1] - t.curv_d[k], lam_c, t.curv_d[k])
        one = fma(-k_r, d, 1.0)
        cos_t, tan_t = np.cos(theta_cl), np.tan(theta_cl)
        if contracted:
            ratio = cos_t / one
            kappa = fma(fma(fma(k_r_d, d, k_r * dp), tan_t, dpp), (ratio * ratio) * cos_t, k_r * ratio)
            v = (sd * one) / cos_t
            a = fma((sd * sd) / cos_t, fma(one * tan_t, fma(kappa, one / cos_t, -k_r), -fma(k_r, dp, k_r_d * d)), sdd * (one / cos_t))
        else:
            kappa = (dpp + (k_r * dp + k_r_d * d) * tan_t) * cos_t * (cos_t / one) ** 2 + (cos_t / one) * k_r
            v = sd * (one / cos_t)
            a = sdd * one / cos_t + ((sd ** 2) / cos_t) * (one * tan_t * (kappa * one / cos_t - k_r) - (k_r_d * d + k_r * dp))
        tan = t.tan if hasattr(t, "tan") else frontend.compute_vertex_tangents(t.ref)
        px, py = fma(lam, t.ref[k + 1, 0] - t.ref[k, 0], t.ref[k, 0]), fma(lam, t.ref[k + 1, 1] - t.ref[k, 1], t.ref[k, 1])
        ax, ay = fma(lam, tan[k + 1, 0] - tan[k, 0], tan[k, 0]), fma(lam, tan[k + 1, 1] - tan[k, 1], tan[k, 1])
        tn2 = fma(ax, ax, ay * ay)
        if defect == "rsqrt_f32":
            inv = (np.float32(1.0) / np.sqrt(tn2.astype(np.float32))).astype(np.float64)
            x, y = px - d * (ay * inv), py + d * (ax * inv)
        elif contracted:
            inv = 1.0 / np.sqrt(tn2)
            x, y = fma(-d, ay * inv, px), fma(d, ax * inv, py)
        else:
            tn = np.sqrt(tn2)
            x, y = px - d * (ay / tn), py + d * (ax / tn)
        before = kappa[:, :-1].copy()
        if defect == "carry_f32":   # what one chunk hands the next
            edge = np.arange(CHUNK - 1, n - 1, CHUNK)
            before[:, edge] = _f32(before[:, edge])
        kappa_dot = np.concatenate((np.zeros((K, 1)), kappa[:, 1:] - before), axis=1)
    return np.stack((x, y, theta, v, a, kappa, kappa_dot, theta_cl), axis=1)


def restated_cost(cost, rows, planes, lengths, how):
    """``_score.cost_of`` on restated rows [K, 8, n] with its sums taken another way: "reversed" (the honest variant: last pose first) or
    "f32" (the planted defect: terms in double, partial sums in float32)"""
    K, n = rows.shape[0], rows.shape[2]
    lengths = np.full(K, n) if lengths is None else np.asarray(lengths)

    def total(term):
        if how == "f32":
            acc = np.float32(0.0)
            for q in term:
                acc = np.float32(acc + np.float32(q))
            return float(acc)
        acc = 0.0
        for q in term[::-1]:
            acc = acc + q
        return acc
    out = np.full(K, np.nan)
    for k in range(K):
        m = int(lengths[k])
        a, v, th, s, d = rows[k, 4, :m], rows[k, 3, :m], rows[k, 7, :m], planes[0][k, :m], planes[3][k, :m]
        tail = total((0.25 * np.abs(th)) ** 2) + (5 * abs(th[-1])) ** 2
        if int(cost.kind) == COST_FAILSAFE:
            out[k] = total(a ** 2) + total((0.25 * d) ** 2) + (20 * d[-1]) ** 2 + tail
            continue
        c = total((cost.w_a * a) ** 2)
        if not math.isnan(cost.desired_speed):
            c += total((5 * (v - cost.desired_speed)) ** 2) + 50 * (v[-1] - cost.desired_speed) ** 2 + 100 * (v[m // 2] - cost.desired_speed) ** 2
        if not math.isnan(cost.desired_s):
            c += total((0.25 * (cost.desired_s - s)) ** 2) + (20 * (cost.desired_s - s[-1])) ** 2
        out[k] = c + total((0.25 * (cost.desired_d - d)) ** 2) + (20 * (cost.desired_d - d[-1])) ** 2 + tail
    return out


# ---- the device ------------------------------------------------------------------------------------------------------------------
def run_lift(lf, c, path=None):
    lf.set_reference(*L.table_args(path or c.path))
    return lf.lift(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)


def run_pick(pk, c, cost):
    """rp_pick_select with mode = 0: no collision test"""
    pk.set_reference(*L.table_args(c.path))
    pk.set_obstacles(None)
    return pk.pick(c.p, cost, *c.planes, lengths=c.lengths, theta0=c.theta0, poses=False, swept=False, want_planes=True)


def run_epick(ep, c, cost):
    """rp_epick_select with mode = 0 and one empty member"""
    ep.set_reference(*L.table_args(c.path))
    ep.set_static(None)
    ep.set_members(np.full((1, 0, 0, 5), np.nan), 0)
    return ep.pick(c.p, cost, *c.planes, lengths=c.lengths, theta0=c.theta0, poses=False, swept=False, want_planes=True)


# Planes of rp_lift_evaluate on a case's own tables that exceed the rule on an MI355X: (case, plane) -> diagnosis.  tests/test_liftx.py
# asserts each on its own, expected to fail, strictly; every other plane of that comparison, and every plane on the padded tables and
# every cost, is asserted as usual: they have no entry here.
KNOWN_EXCEEDANCES = {}


def cpu_lines():
    lines = []
    for name in CASE_NAMES:
        c = case(name)
        rows, n_out, _ = cpu_rows(name)
        K, n = c.planes[0].shape
        lines.append(f"{name}  {K} x {n}, {len(c.path.pos) - 1} segments, {n_out} left out")
        lines += [f"  {r.row:>9s} scale {r.scale:9.3e}  E_O {r.e_o:9.3e}  R_O {r.r_o:9.3e}" for r in rows]
        for q, cost in enumerate(c.costs):
            sel = cost_selection(name)
            e_o = compare_costs(reference(name).cost[q], oracle_view(name)[1 + q], oracle_view(name)[1 + q], sel, c.out.lengths)[0]
            lines.append(f"  cost ({'fail-safe' if cost.kind == COST_FAILSAFE else 'default'}) of {int(sel.sum())} feasible trajectories: oracle {e_o:9.3e} relative")
    return lines


def device_lines():
    """per case and library: E_D, R_D, their ratios to the oracle's and the bounds (tests/test_liftx.py asserts them)"""
    from commonroad_rp_amd import EnsemblePicker, TrajectoryLifter, TrajectoryPicker
    lines, bad, known = [], 0, 0
    with TrajectoryLifter(0) as lf, TrajectoryPicker(0) as pk, EnsemblePicker(0) as ep:
        for name in CASE_NAMES:
            c, ref, ov = case(name), reference(name), oracle_view(name)
            runs = [("rp_lift_evaluate", stacked(run_lift(lf, c)))]
            if fits_both(name):
                runs += [(f"rp_lift_evaluate, {q} segments", stacked(run_lift(lf, c, padded(c.path, q)))) for q in (LDS_ROWS, LDS_ROWS + 1)]
            seen = {}
            for what, got in runs:
                rows, n_out, _ = compare_planes(ref.rows, ov[0], got)
                text = []
                for r in rows:
                    is_known = not r.ok and what == "rp_lift_evaluate" and (name, r.row) in KNOWN_EXCEEDANCES
                    text.append("  " + r.line() + (" (known)" if is_known else ""))
                    bad, known = bad + ((not r.ok) and not is_known), known + is_known
                if tuple(text) in seen:   # (a variant whose figures are those of an earlier one is named only)
                    lines.append(f"{name}  {what}: the figures of {seen[tuple(text)]}")
                else:
                    lines += [f"{name}  {what}  ({n_out} left out)"] + text
                seen.setdefault(tuple(text), what)
            for q, cost in enumerate(c.costs):
                for lib, got in (("rp_pick_select", run_pick(pk, c, cost)), ("rp_epick_select", run_epick(ep, c, cost))):
                    same = all(np.array_equal(getattr(got, pl).view(np.uint64), runs[0][1][:, j].copy().view(np.uint64)) for j, pl in enumerate(PLANES))
                    e_o, e_d, bound, ok = compare_costs(ref.cost[q], ov[1 + q], got.cost, cost_selection(name), c.out.lengths)
                    lines.append(f"{name}  {lib} {'fail-safe' if cost.kind == COST_FAILSAFE else 'default'} cost: oracle {e_o:9.3e} device {e_d:9.3e} bound {bound:9.3e} "
                                 f"relative; planes {'bit-equal to the lift' if same else 'DIFFER from the lift'}{'' if ok else '   EXCEEDS'}")
                    bad += (not ok) + (not same)
    return lines + ["", f"{bad} bounds exceeded, {known} known exceedances"], bad


def main(argv):
    if not X.HAVE_LONGDOUBLE:
        print(X.SKIP_REASON)
        return 1
    path = argv[1] if len(argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "accuracy_lift.txt")
    lines = ["The lifted planes against the extended-precision reference (tests/_liftx.py).  First the CPU table: per case and plane the scale,",
             "the largest and the root-mean-square distance of the double oracle (tests/_lift.reference) to the reference (E_O, R_O), and the",
             "trajectories left out.  Then, from a machine with a GPU, per case and library the device's E_D, R_D, the ratio device / oracle",
             "in brackets and the bound it is held to (tests/test_liftx.py); rp_pick_select and rp_epick_select: the cost, and that their",
             "planes have the bits of the lift's.  A table variant whose figures are those of an earlier one is named only.", ""]
    lines += cpu_lines() + [""]
    bad = 0
    try:   # a session cannot be made: no library or no GPU, the CPU table alone.  Whatever fails behind this point is a failure.
        from commonroad_rp_amd import TrajectoryLifter
        TrajectoryLifter(0).close()
        have_device = True
    except (RpLibraryMissing, RpError) as e:
        have_device = False
        lines.append(f"(no device columns: {type(e).__name__}: {e})")
    if have_device:
        dev, bad = device_lines()
        lines += dev
    text = "\n".join(lines) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
