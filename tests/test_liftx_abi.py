"""What tests/test_liftx.py (GPU) rests on, checked without a GPU: that generalising ``_xref._from_planes`` changed no bit of what
``_xref`` hands out, that the double oracle of the lift (``_lift.reference``) stays within 1e-11 of the extended-precision reference
(``_liftx.evaluate``) on every case with no trajectory left out of the existing cases and at most 2 % of a new family's, that the new
families meet the conditions they state, and that the comparison has teeth: planted defects the earlier 1e-6 / 1e-9 contract cannot
see exceed the rule, the honest restatement with its sums reassociated and fma contracted does not."""
import numpy as np
import pytest

import _dd as dd
import _lift as L
import _liftx as LX
import _xref as X
from _dd import DD

pytestmark = pytest.mark.skipif(not X.HAVE_LONGDOUBLE, reason=X.SKIP_REASON)
LD = X.LD
TIGHT = ("x", "y", "theta", "theta_cl")   # lengths and angles: 1e-9 in the earlier contract, the other planes 1e-6


# ---- 1. the refactor of tests/_xref.py is bit-neutral ---------------------------------------------------------------------------------
def _from_planes_before(c, s, s_vel, s_acc, d, d_vel, d_acc, tl):
    """``_xref._from_planes`` as it stood before ``_xref.per_pose`` was taken out of it, kept to compare bits with"""
    _dd_in, _valid_orientation, _tangents, _enlarge, _cost = X._dd_in, X._valid_orientation, X._tangents, X._enlarge, X._cost
    p, tb, cst = c.inp.params, c.tables, c.inp.cost
    n, m = p.N + 1, len(tl)
    dt = DD(LD(p.dt))
    low = bool(p.low_vel_mode)
    valid = np.arange(n)[None, :] < tl[:, None]
    z = lambda a: dd.where(valid, a, 0)
    s_vel = dd.where(abs(s_vel) < DD(X.EPS), 0, s_vel)
    d_vel = dd.where(abs(d_vel) < DD(X.EPS), 0, d_vel)
    moving = s_vel > DD(X.S_VEL_MIN)
    if not low:
        safe = dd.where(moving, s_vel, 1)
        dp = dd.where(moving, d_vel / safe, 0)
        dpp = dd.where(moving, (d_acc - dp * s_acc) / (safe * safe), 0)
    else:
        dp, dpp = d_vel, d_acc
    rp, rth, rk, rkd = (_dd_in(a) for a in (tb.ref_pos, tb.ref_theta, tb.ref_curv, tb.ref_curv_d))
    nr = len(tb.ref_pos)
    k = np.clip(np.searchsorted(rp.hi, s.hi, side="right") - 1, 0, nr - 2)
    k = np.clip(np.where(s < rp[k], k - 1, k), 0, nr - 2)
    seg = rp[k + 1] - rp[k]
    lam = (s - rp[k]) / seg
    th_ref = _valid_orientation((rth[k + 1] - rth[k]) * (s - rp[k]) / seg + rth[k])
    theta_cl = dd.atan(dp)
    theta = theta_cl + th_ref
    use = moving | low
    if not use[valid].all():
        theta = theta.copy()
        for i in range(n):
            prev = dd.broadcast_to(DD(LD(p.x0_orientation)), (m,)) if i == 0 else theta[:, i - 1]
            theta[:, i] = dd.where(use[:, i], theta[:, i], prev)
        theta_cl = dd.where(use, theta_cl, theta - th_ref)
    k_r = (rk[k + 1] - rk[k]) * lam + rk[k]
    k_r_d = (rkd[k + 1] - rkd[k]) * lam + rkd[k]
    one_krd = 1 - k_r * d
    sin_t, cos_t = dd.sincos(theta_cl)
    tan_t = sin_t / cos_t
    kappa = (dpp + (k_r * dp + k_r_d * d) * tan_t) * cos_t * (cos_t / one_krd) ** 2 + (cos_t / one_krd) * k_r
    v = s_vel * (one_krd / cos_t)
    a = s_acc * one_krd / cos_t + ((s_vel * s_vel) / cos_t) * (one_krd * tan_t * (kappa * one_krd / cos_t - k_r) - (k_r_d * d + k_r * dp))
    tx, ty = _tangents(tb)
    rx, ry = _dd_in(tb.ref_x), _dd_in(tb.ref_y)
    px, py = rx[k] + lam * (rx[k + 1] - rx[k]), ry[k] + lam * (ry[k + 1] - ry[k])
    ax, ay = tx[k] + lam * (tx[k + 1] - tx[k]), ty[k] + lam * (ty[k + 1] - ty[k])
    tn = dd.sqrt(ax * ax + ay * ay)
    x, y = px - d * (ay / tn), py + d * (ax / tn)
    st = {X.X: z(x), X.Y: z(y), X.THETA: z(theta), X.V: z(v), X.A: z(a), X.KAPPA: z(kappa), X.S: z(s), X.D: z(d), X.THETA_CL: z(theta_cl),
          X.S_DOT: z(s_vel), X.S_DDOT: z(s_acc), X.D_DOT: z(d_vel), X.D_DDOT: z(d_acc)}
    kd = dd.zeros((m, n))
    kd[:, 1:] = st[X.KAPPA][:, 1:] - st[X.KAPPA][:, :-1]
    st[X.KAPPA_DOT] = kd
    _enlarge(st, tl, n, dt)
    inter = {key: val.ld() for key, val in dict(s=s, d=d, dp=dp, dpp=dpp, k_r=k_r, k_r_d=k_r_d, theta_cl=theta_cl, one_krd=one_krd, cos=cos_t).items()}
    return np.stack([st[r].ld() for r in range(14)], axis=1), _cost(cst, st, n).ld(), inter


def _same_longdoubles(a, b):
    """bit-equal as numbers, NaN in the same places (the bytes of a longdouble carry padding)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all()) and bool((np.signbit(a) == np.signbit(b)).all())


@pytest.mark.parametrize("name", ("arc_keep_n17", "scurve_stop_n64", "arc_low_n65"))
def test_xref_hands_out_the_bits_it_did_before(name, monkeypatch):
    """``_xref.evaluate`` (what ``_xref.reference`` caches) and ``_xref.evaluate_planes`` (what tests/_kin_plan.py reads): states, costs
    and every intermediate they had, through the code path of before and through ``_xref.per_pose``"""
    import _kin_plan
    c = X.case(name)
    lon, lat, tl, _ = X.sample(c.inp, X.subset(name))
    planes, ptl = _kin_plan.lift_planes(name)
    now = X.evaluate(c, lon, lat, tl), X.evaluate_planes(c, planes, ptl)
    assert _same_longdoubles(now[0][0], X.reference(name).states) and _same_longdoubles(now[0][1], X.reference(name).cost)
    monkeypatch.setattr(X, "_from_planes", _from_planes_before)
    before = X.evaluate(c, lon, lat, tl), X.evaluate_planes(c, planes, ptl)
    for (st_n, cost_n, inter_n), (st_b, cost_b, inter_b) in zip(now, before):
        assert _same_longdoubles(st_n, st_b) and _same_longdoubles(cost_n, cost_b)
        assert set(inter_b) <= set(inter_n) and all(_same_longdoubles(inter_n[k], inter_b[k]) for k in inter_b)


def test_reference_is_the_xref_evaluation_without_the_extension():
    """On the planes of an ``_xref`` case the new entry point gives the rows ``_xref.evaluate_planes`` gives below each length, bit for
    bit; for a candidate that fills the horizon (no extension) the cost over its own length is ``_xref``'s cost"""
    import _kin_plan
    name = "arc_keep_n17"
    c, lc, ref = X.case(name), LX.case("xref:" + name), LX.reference("xref:" + name)
    planes, tl = _kin_plan.lift_planes(name)
    states, cost, _ = X.evaluate_planes(c, planes, tl)
    n = states.shape[2]
    valid = np.arange(n)[None, :] < tl[:, None]
    for q, row in enumerate(LX.ROWS14):
        assert _same_longdoubles(np.where(valid, ref.rows[:, q], 0), np.where(valid, states[:, row], 0)), LX.PLANES[q]
    full = tl == n
    assert full.sum() >= 4 and lc.costs[0] is c.inp.cost
    assert _same_longdoubles(ref.cost[0][full], cost[full])


# ---- 2. the oracle on every case --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LX.CASE_NAMES)
def test_oracle_within_1e11_of_the_reference_and_the_left_out_caps(name, capsys):
    c = LX.case(name)
    rows, n_out, out = LX.cpu_rows(name)
    K = c.planes[0].shape[0]
    with capsys.disabled():
        print(f"\n{name}: {K} trajectories, {n_out} left out")
        for r in rows:
            print(f"  {r.row:>9s} scale {r.scale:9.3e}  E_O {r.e_o:9.3e}  R_O {r.r_o:9.3e}")
    assert n_out <= (LX.LEFT_OUT_CAP_NEW * K if c.family == "c" else 0), (name, n_out)
    assert max(r.e_o for r in rows) <= X.ORACLE_BOUND, [r.line() for r in rows if r.e_o > X.ORACLE_BOUND]
    assert not X.failures(rows)        # the oracle passes its own comparison
    compared = np.isfinite(LX.oracle_view(name)[0])
    assert compared.any(axis=(1, 2)).sum() >= K - (3 if name in ("lift:nan_input", "lift:off_start") else 0)   # (trajectories that are off from pose 0)
    assert (c.family == "a") == (not c.costs)
    for q, cost in enumerate(c.costs):
        sel = LX.cost_selection(name)
        cX, cO = LX.reference(name).cost[q], LX.oracle_view(name)[1 + q]
        assert sel.sum() >= 2 and (cX[sel] > 0).all()
        e_o, _, bound, ok = LX.compare_costs(cX, cO, cO, sel, c.out.lengths)
        assert e_o <= X.ORACLE_BOUND and ok


def test_the_cost_cases_have_both_kinds():
    from commonroad_rp_amd._capi import COST_DEFAULT, COST_FAILSAFE
    for name in LX.COST_CASES:
        assert [int(k.kind) for k in LX.case(name).costs] == [COST_DEFAULT, COST_FAILSAFE], name
    assert {"xref:" + n for n in ("arc_keep_n17", "scurve_stop_n64", "arc_low_n65", "scurve_keep_n111", "scurve_still002_n111", "straight_fast_n111",
                                 "arc_failsafe_n64", "scurve_low_failsafe_n17")} <= set(LX.COST_CASES)
    assert LX.case("xref:arc_failsafe_n64").costs[1] is X.case("arc_failsafe_n64").inp.cost      # the case's own fail-safe cost


# ---- 3. the new families meet their conditions ------------------------------------------------------------------------------------------
def test_new_families_meet_their_conditions():
    for name in LX.NEW_FAMILIES:
        c = LX.case(name)
        assert c.planes[0].shape[0] <= 16 and c.p.constraint_mask == 0 and (c.out.status == 1).all(), name
        assert LX.compared_poses(name).sum() == (c.out.lengths.sum()), name     # nothing leaves its path
    # wrapped: clear of the wrap, beyond pi, and crossing it inside a chunk and across a chunk boundary
    assert LX.wrap_distance("wrapped") >= LX.WRAP_CLEAR
    th = LX.reference("wrapped").inter["th_table"]
    assert (th[:4] > np.pi).all() and (th[:4] < 2 * np.pi).all() and LX.case("wrapped").planes[0][:4].min() >= 70.0 and LX.case("wrapped").planes[0].max() <= 140.0
    assert LX.wrap_crossings("wrapped") == [(4, 64), (5, 21)]
    assert np.abs(LX.case("wrapped").planes[3]).max() <= 0.008
    # three_chunks: where the standstills start, where the rows end
    assert LX.standstill_starts("three_chunks_130") == [(0, 126), (1, 127), (2, 128)]
    assert LX.standstill_starts("three_chunks_193") == [(0, 126), (0, 191), (1, 127), (1, 191)]
    assert list(LX.case("three_chunks_130").lengths) == [130, 129, 130]
    moving_again = LX.case("three_chunks_193").planes[1][:, 131:191]
    assert (moving_again[:, 1:] > 0.001).all()                                    # ... and move on into the fourth chunk
    assert np.abs(LX.reference("three_chunks_193").inter["k_r"]).max() > 1e-3     # a curved path
    # tight: 1 - k_r d from 1 down to about 1/6, beyond 1.8 outside; coordinates of 3e3
    for name in ("tight_hv", "tight_lv"):
        one = LX.reference(name).inter["one_krd"]
        assert one[0].max() >= 0.99 and one[0].min() <= 1.01 and 0.16 <= one.min() <= 0.19 and one.max() >= 1.8, (name, one.min(), one.max())
        assert 2.0e3 <= np.abs(LX.reference(name).rows[:, :2]).max() <= 3.1e3
    assert LX.case("tight_lv").p.low_vel_mode == 1 and LX.case("tight_hv").p.low_vel_mode == 0
    # steep: theta_cl up to +-1.4995 rad in low-velocity mode; s_dot next to 0.001 on both sides in high-velocity mode
    th_cl = LX.reference("steep_lv").rows[:, 7]
    assert LX.case("steep_lv").p.low_vel_mode == 1 and th_cl.max() >= 1.499 and th_cl.min() <= -1.499 and (th_cl[0] == 0).all()
    assert np.abs(LX.case("steep_lv").planes[4]).max() == 14.0
    assert LX.rule_distance("steep_hv") >= LX.RULE_CLEAR and LX.rule_distance("steep_lv") >= LX.RULE_CLEAR
    sd = LX.case("steep_hv").planes[1][:, 0]
    assert sd[0] > 0.001 and sd[0] - 0.001 <= 2e-12 and sd[5] < 0.001 and 0.001 - sd[5] <= 2e-12 and sd.max() == 0.01
    assert LX.standstill_starts("steep_hv") == [(5, 0)]
    assert np.abs(LX.reference("steep_hv").inter["dp"]).max() >= 9.9


def test_cases_reach_what_they_claim():
    """worked out from the inputs: a standstill's carry that starts on lane 63 and on lane 0 (at pose 0, reading theta0, and behind a
    chunk boundary), a wrap of the table heading between two poses of one chunk and across a chunk boundary, both table variants"""
    got = vars(LX.coverage())
    assert all(got.values()), got
    assert [n for n in LX.CASE_NAMES if LX.fits_both(n)] == list(LX.BOTH_VARIANTS)


@pytest.mark.parametrize("name", ("lift:n65", "xref:arc_keep_n17", "tight_lv"))
def test_a_straight_tail_changes_neither_reference(name):
    """what lets the GPU test reuse X and O on the padded paths: a tail moves the end tangent of the last segment alone, which no pose
    of a case that ``fits_both`` reaches"""
    c = LX.case(name)
    assert LX.fits_both(name)
    for n_seg in (LX.LDS_ROWS, LX.LDS_ROWS + 1):
        t = LX.padded(c.path, n_seg)
        assert len(t.pos) - 1 == n_seg
        assert _same_longdoubles(LX.evaluate(c.p, t, c.planes, c.lengths, c.theta0).rows, LX.reference(name).rows)
        o = LX.stacked(L.reference(c.p, t, *c.planes, lengths=c.lengths, theta0=c.theta0))
        np.testing.assert_array_equal(o.view(np.uint64), LX.oracle_view(name)[0].view(np.uint64))


# ---- 4. the rule has teeth -------------------------------------------------------------------------------------------------------------
def _earlier_contract_holds(O, D):
    """tests/test_lift.py's tolerances: 1e-9 for x, y, theta, theta_cl, 1e-6 for v, a, kappa, kappa_dot, where O holds a number"""
    fin = np.isfinite(O)
    worst = [float(np.abs(np.where(fin[:, r], D[:, r] - O[:, r], 0.0)).max()) for r in range(8)]
    return all(w <= (L.TOL if LX.PLANES[r] in TIGHT else L.STATE_ATOL) for r, w in enumerate(worst))


def _restated(name, **how):
    c = LX.case(name)
    return LX.restate(c.p, c.path, c.planes, c.theta0, **how)


@pytest.mark.parametrize("name", LX.CASE_NAMES)
def test_honest_restatement_is_within_the_rule(name):
    """the lift's formulas in NumPy doubles, as written and with fma contracted and sums and products associated the other way"""
    for contracted in (False, True):
        rows, _, _ = LX.compare_planes(LX.reference(name).rows, LX.oracle_view(name)[0], _restated(name, contracted=contracted))
        assert not X.failures(rows), "\n".join([f"{name} contracted={contracted}"] + X.failures(rows))
    c = LX.case(name)
    for q, cost in enumerate(c.costs):
        got = LX.restated_cost(cost, _restated(name, contracted=True), c.planes, c.lengths, "reversed")
        e_o, e_d, bound, ok = LX.compare_costs(LX.reference(name).cost[q], LX.oracle_view(name)[1 + q], got, LX.cost_selection(name), c.out.lengths)
        assert ok, (name, q, e_o, e_d, bound)


# defect -> (the cases it must exceed the rule on while the earlier contract holds, the planes it must be seen on)
PLANTED = {
    "rcp_f32": (("wrapped", "xref:scurve_stop_n64", "lift:standstill_across"), {"theta", "theta_cl", "kappa"}),             # the reciprocal of s_dot
    "atan_f32": (("wrapped", "xref:scurve_stop_n64", "xref:straight_stop_n65"), {"theta", "theta_cl"}),
    "lam_f32_curvature": (("three_chunks_130", "three_chunks_193", "lift:n65", "xref:scurve_keep_n111"), {"kappa"}),      # lam of the curvature interpolation only
    "rsqrt_f32": (("wrapped",), {"x", "y"}),                                                                            # the tangent length
    "carry_f32": (("three_chunks_130", "three_chunks_193", "lift:n65", "lift:n129"), {"kappa_dot"}),                     # kappa across a chunk boundary
    "cost_sums_f32": (("wrapped", "xref:arc_failsafe_n64", "three_chunks_193"), {"cost"}),                              # the cost's partial sums, both kinds
}


@pytest.mark.parametrize("defect", list(PLANTED))
def test_planted_defects_exceed_the_rule(defect):
    names, planes = PLANTED[defect]
    assert set(PLANTED) == set(LX.DEFECTS)
    for name in names:
        O = LX.oracle_view(name)[0]
        D = _restated(name, defect=defect)
        assert _earlier_contract_holds(O, D), (defect, name)          # the 1e-6 / 1e-9 contract cannot see it
        if defect == "cost_sums_f32":   # the planes are the honest ones; the sums are not
            c = LX.case(name)
            np.testing.assert_array_equal(D, _restated(name))
            for q, cost in enumerate(c.costs):
                got = LX.restated_cost(cost, D, c.planes, c.lengths, "f32")
                e_o, e_d, bound, ok = LX.compare_costs(LX.reference(name).cost[q], LX.oracle_view(name)[1 + q], got, LX.cost_selection(name), c.out.lengths)
                assert not ok and e_d > 100 * bound, (name, q, e_o, e_d, bound)
            continue
        rows, _, _ = LX.compare_planes(LX.reference(name).rows, O, D)
        seen = {r.row for r in rows if not r.ok}
        assert planes <= seen, (defect, name, [r.line() for r in rows])
    if defect == "carry_f32":   # ... and moves nothing where no chunk boundary is crossed
        for name in ("lift:n63", "lift:n64"):
            np.testing.assert_array_equal(_restated(name, defect=defect), _restated(name))
    if defect == "lam_f32_curvature":
        assert np.array_equal(_restated("lift:n65", defect=defect)[:, :3], _restated("lift:n65")[:, :3])     # x, y, theta keep the double lam
