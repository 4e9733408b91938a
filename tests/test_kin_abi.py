"""What tests/test_kin.py rests on, checked without a GPU: every case of tests/_kin.py meets the conditions of a case (the placed
margin outside 8 B, every other margin outside 1e-6 scale; nothing dropped), the double-word reference agrees with a 50-digit
evaluation, the guard band B = 16 u scale is at least 8 times the largest margin at which the double restatements (tests/_score.py,
oracle/rp_oracle.c) decide otherwise, the arithmetic include/rp_score.h documents gives the reference's verdict on every case, and every
planted defect of that arithmetic turns its families red and no other."""
import time

import numpy as np
import pytest

import _kin as K
import _lift
import _score as S

pytestmark = pytest.mark.skipif(not K.HAVE_LONGDOUBLE, reason=K.SKIP_REASON)

GROUPS = (("std", False), ("tan", False), ("std", True))


def test_math_tan_and_numpy_tan_differ_on_the_second_vehicle():
    import math
    x = K.tan_delta()
    assert x is not None and 0.2 < x < 1.3 and math.tan(x) != float(np.tan(x))
    assert set(K.vehicles()) == {"std", "tan"}


def test_numpy_rounds_half_to_even_at_five_digits():
    """``round(yaw_rate, 5)`` of the reference is NumPy's scale-rint-unscale: recorded, since the reference inherits it."""
    print("numpy", np.__version__, "round(np.float64(2.5e-05), 5) =", round(np.float64(2.5e-05), 5))
    assert round(np.float64(2.5e-05), 5) == 2e-05
    assert np.rint(2.5e-05 * 1e5) / 1e5 == 2e-05


def test_case_list_is_complete_and_quick_to_build():
    t0 = time.time()
    built = [K.group.__wrapped__(name, lift) for name, lift in GROUPS]
    took = time.time() - t0
    print(f"three groups and their references: {took:.2f} s; K = {[g.K for g in built]}")
    assert took < 5.0
    std, tan, lift = built
    assert set(std.family) == set(K.FAMILIES) and set(tan.family) == {"kappa", "yaw_bound"} and set(lift.family) == set(K.LIFT_FAMILIES)
    assert 200 <= std.K <= 400 and std.v.shape == (std.K, K.N_POSES)
    for fam in ("kappa", "acc_switch", "kappa_dot", "yaw_bound", "yaw_half"):      # both signs at all three displacements
        rows = [r for r in std.rows if r.family == fam]
        for level in ("64B", "65536B", "1e-6"):
            assert {r.sign for r in rows if r.level == level} == {1, -1}, (fam, level)
    deciding = {int(r.step) for r in std.rows}
    assert set(K.STEPS) <= deciding
    assert {r.pair for r in std.rows if r.family == "priority"} == set(K.PAIRS)
    assert sum(r.family == "priority" for r in std.rows) == 3 * len(K.PAIRS)
    assert sum(r.family == "nonfinite" for r in std.rows) == 14
    big = [k for k, r in enumerate(std.rows) if r.level == "kappa=1e+200"][0]    # the overflow the documented arithmetic passes at its own step
    assert std.want[K.BIT["kappa_dot"]][big] == S.status_word(2, K.REASON["kappa_dot"], int(std.rows[big].step) + 1)
    ties = [r for r in std.rows if r.family == "yaw_tie"]
    assert {r.sign for r in ties} == {1, -1} and len(ties) == 12                     # even and odd k
    for r in ties:                                                                   # the doubles the family is about
        x = ((r.theta[r.step] - r.theta[r.step - 1]) / std.veh.dt) * 1e5
        assert abs(x) % 1.0 == 0.5
    # every row but ``where`` hands its successor's first pose on; ``where`` is filled with violations behind the end
    for k, r in enumerate(std.rows):
        if r.family != "where" or r.L == K.N_POSES:
            continue
        assert std.kappa[k, r.L] == 50.0 and std.v[k, r.L] == -5.0 and std.a[k, r.L] == 100.0


@pytest.mark.parametrize("name,lift", GROUPS)
def test_every_case_meets_the_conditions_of_a_case(name, lift):
    g = K.group(name, lift)
    bad = K.margin_failures(g)
    assert not bad, bad[:10]


@pytest.mark.parametrize("name,lift", GROUPS)
def test_own_mask_full_mask_and_cleared_bit(name, lift):
    """"+" is feasible and "-" carries its check and step under the mask of its check alone; with the bit cleared the "-" version gives
    what its "+" twin gives under the full mask (feasible wherever that one is)."""
    g = K.group(name, lift)
    seen = 0
    for k, r in enumerate(g.rows):
        c = K.own_check(r)
        if c is None:
            continue
        seen += 1
        want = 1 if r.sign > 0 else S.status_word(2, K.REASON[c], int(r.step))
        assert g.want[K.BIT[c]][k] == want, (k, r.family, r.level, r.sign)
        cleared = int(g.want[K.FULL & ~K.BIT[c]][k])
        assert (cleared >> 4) & 7 != K.REASON[c]
        if r.sign < 0 and r.family not in ("v_edge", "a_edge", "yaw_tie") and r.level != "branch":
            twin = g.rows[k - 1]
            assert (twin.family, twin.level, twin.sign) == (r.family, r.level, 1)     # (its own deciding step: the steps rotate)
            if g.want[K.FULL][k - 1] == 1:
                assert cleared == 1, (k, r.family, r.level)
    assert seen == sum(K.own_check(r) is not None for r in g.rows) >= 60
    feasible_plus = sum(g.want[K.FULL][k] == 1 for k, r in enumerate(g.rows) if r.sign > 0 and K.own_check(r))
    assert feasible_plus >= 25


def test_selection_does_not_hang_on_the_rounding_of_a_cost():
    for name in K.vehicles():
        g = K.group(name)
        for m in K.MASKS:
            best, n_feasible, counts = K.selection(g, m)
            assert best >= 0 and n_feasible + counts.sum() == g.K
            assert K.runner_up_gap(g, m) > 1e-9, (name, m)


def test_reference_against_fifty_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    g = K.group("std")
    veh, ex = g.veh, g.exact
    F = mp.mpf
    kmax = mp.tan(F(veh.delta_max)) / F(veh.wheelbase)
    worst, checked = 0.0, 0
    for k in range(0, g.K, 3):
        r = g.rows[k]
        if r.doc:
            continue
        for i in sorted({int(r.step), max(int(r.step) - 1, 0), min(int(r.step) + 1, r.L - 1)}):
            v, a, kp, th = (F(float(q[k, i])) for q in (g.v, g.a, g.kappa, g.theta))
            kp0, th0 = F(float(g.kappa[k, i - 1])) if i else kp, F(float(g.theta[k, i - 1])) if i else th
            y = (th - th0) / F(veh.dt) * 100000
            fl = mp.floor(y)
            rr = fl + (1 if y - fl > F("0.5") else 0 if y - fl < F("0.5") else int(fl) % 2)
            hi = F(veh.a_max) * F(veh.v_switch) / v if v > F(veh.v_switch) else F(veh.a_max)
            want = {"velocity": v + F(1e-5), "kappa": kmax - abs(kp), "yaw_rate": kmax * v - abs(rr) / 100000,
                    "kappa_dot": F(veh.v_delta_max) * (1 + (F(veh.wheelbase) * kp) ** 2) / F(veh.wheelbase) - abs((kp - kp0) / F(veh.dt)),
                    "acceleration": min(a + F(veh.a_max), hi - a)}
            for c in K.CHECKS:
                got = F(ex.g[c][k, i].astype(np.float64)) + F(float(ex.g[c][k, i] - np.longdouble(ex.g[c][k, i].astype(np.float64))))
                err = abs(got - want[c]) / F(max(float(ex.scale[c][k, i]), 1e-300))
                worst = max(worst, float(err))
                assert (want[c] < 0) == bool(ex.fail[c][k, i]), (k, i, c)
                checked += 1
    print(f"{checked} margins, largest |double-word - 50 digits| / scale: {worst:.1e}")
    assert checked >= 1000 and worst <= 2.0 ** -62      # (the margin is reported rounded to longdouble; its sign comes from both words)


def test_guard_band_is_eight_times_the_double_forms_largest_wrong_margin():
    m = K.measured()
    for who in ("restatement", "oracle", "documented"):
        print(who, {c: round(float(x), 3) for c, x in m[who].items()})
        for c, worst in m[who].items():
            assert K.BAND >= 8.0 * worst, (who, c, worst)
    lad = K.ladder()
    near = sum(int((np.abs(lad.exact.g[c][lad.check == c, 1]).astype(float) <= 4 * K.U * lad.exact.scale[c][lad.check == c, 1]).sum())
               for c in ("kappa", "yaw_rate", "kappa_dot", "acceleration"))
    assert near >= 4000       # the ladder does reach the last few ulp
    assert max(max(x.values()) for x in m.values()) > 0.0   # ... where the double forms do decide otherwise


def _red(defect):
    red = set()
    for name in K.vehicles():
        g = K.group(name)
        fail = K.documented(g.veh, g.v, g.a, g.kappa, g.theta, defect=defect)
        for m in K.MASKS:
            st = K.status_words(fail, g.lengths, m, reverse=defect == "reversed_chain")
            red |= set(g.family[st != g.want[m]])
    return red


def test_documented_arithmetic_gives_the_reference_verdict_on_every_case():
    assert _red(None) == set()
    g = K.group("std", lift=True)
    fail = K.documented(g.veh, g.v, g.a, g.kappa, g.theta)
    for m in K.LIFT_MASKS:
        np.testing.assert_array_equal(K.status_words(fail, g.lengths, m), g.want[m])


# the families a defect must turn red, and no other.  ">=": the bounds that are met exactly (inf >= inf among them); the reversed chain:
# every family in which two checks fail in one step (v below -1e-5 also fails the yaw-rate check, a spike of kappa also kappa_dot)
EXPECTED_RED = {
    "ge_for_gt": {"v_edge", "a_edge", "yaw_bound", "nonfinite"},
    "v_below_zero": {"v_edge"},
    "kappa_max_float32": {"kappa", "yaw_bound"},
    "trunc_for_rint": {"yaw_bound", "yaw_half", "yaw_tie"},
    "half_away_for_rint": {"yaw_tie"},
    "reciprocal_float32": {"acc_switch"},
    "reversed_chain": {"priority", "v_edge", "nonfinite", "where"},
    "rates_from_predecessor": {"where"},
}


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_planted_defect_turns_its_families_red_and_no_other(defect):
    assert _red(defect) == EXPECTED_RED[defect]


def test_lift_rows_are_copies_of_the_inputs_on_the_straight_path():
    """tier 2, exact placement: the NumPy reference of the lift gives v = s_dot (after its |s_dot| < 1e-5 rule), a = s_ddot,
    kappa = d_ddot bit for bit on the straight path with d_dot = 0, and the verdicts of the exact reference."""
    g = K.group("std", lift=True)
    t = _lift.built_path(K.LIFT_POINTS)
    assert not t.curv.any() and not t.curv_d.any()
    o = _lift.reference(K.lift_params(g.veh, K.FULL), t, **K.lift_inputs(g, K.lift_raw_v()))
    live = np.arange(K.N_POSES)[None, :] < g.lengths[:, None]
    for got, want in ((o.v, g.v), (o.a, g.a), (o.kappa, g.kappa)):
        assert np.array_equal(got[live], want[live])
    assert np.ptp(o.theta[live]) == 0.0
    np.testing.assert_array_equal(o.status, g.want[K.FULL])


def test_lift_edge_rows_decide_without_a_guard():
    """tier 2, input branch edges: the doubles beside 1e-5 and 0.001 take the other branch in the reference (rows that differ), and
    no verdict of these trajectories comes nearer than 1e-6 scale to a bound."""
    c = K.lift_edges()
    o = c.out
    assert K.lift_edge_margins(c) >= K.OTHER
    assert c.K == len(K.EDGE_POSES) * 15 and 63 in K.EDGE_POSES
    by = {(q, what, val): k for k, (q, what, val) in enumerate(c.what)}
    nx = np.nextafter
    for q in K.EDGE_POSES:
        # |s_dot| < 1e-5 reads as 0: v is 0 there, and not beside it
        assert o.v[by[q, "s_dot", nx(1e-5, 0.0)], q] == 0.0 and o.v[by[q, "s_dot", 1e-5], q] > 0.0 and o.v[by[q, "s_dot", nx(-1e-5, 0.0)], q] == 0.0
        assert o.v[by[q, "s_dot", -1e-5], q] < 0.0
        # s_dot > 0.001 moves (theta from d' = d_dot / s_dot); at 0.001 the orientation of the pose before is kept
        assert o.theta[by[q, "s_dot", 0.001], q] == o.theta[by[q, "s_dot", 0.001], q - 1]
        assert abs(o.theta[by[q, "s_dot", nx(0.001, 1.0)], q] - o.theta[by[q, "s_dot", nx(0.001, 1.0)], q - 1]) > 1.0
        # |d_dot| < 1e-5 reads as 0
        assert o.theta_cl[by[q, "d_dot", nx(1e-5, 0.0)], q] == 0.0 and o.theta_cl[by[q, "d_dot", 1e-5], q] > 0.0
        assert o.theta_cl[by[q, "d_dot", nx(-1e-5, 0.0)], q] == 0.0 and o.theta_cl[by[q, "d_dot", -1e-5], q] < 0.0
    assert len(set(o.status)) >= 3 and (o.status == 1).any()


def test_planner_tier_admits_every_check_of_every_case():
    """tier 3 (tests/_kin_plan.py): for each of the five cases and each of the four limits a candidate whose four versions meet the
    conditions of a case in both modes, and the two priority versions; the deltas come from the oracle and the reference alone."""
    import _kin_plan as P
    t0 = time.time()
    steps = set()
    for name in P.CASES + tuple(P.LIFT + q for q in P.LIFT_CASES):
        cases = P.cases(name)
        assert len(cases) == 4 * len(P.LIMIT) + 2, (name, sorted({c.check for c in cases}))
        for c in cases:
            if c.check == "priority":
                assert (c.want[True] & 3) == 2 and c.want[False] == c.want[True]
                continue
            veh = P.vehicle(name, **{c.limit: c.value})
            for draw in (False, True):
                assert not P.admitted(name, c.j, veh, c.mask, draw, (c.step, c.check))
            assert c.want[True] == (1 if c.sign > 0 else S.status_word(2, K.REASON[c.check], c.step)) and 0 < c.step < c.tl
            small, large = P.deltas(name, c.j, c.check)
            assert c.delta == (small if c.level == "small" else large) and 0 < small < large <= 0.05
            steps.add(c.step % 16)
        by_mask = {c.mask: c.want[True] for c in cases if c.check == "priority"}
        assert (by_mask[27] >> 4) & 7 == K.REASON["yaw_rate"] and (by_mask[31] >> 4) & 7 == K.REASON["kappa"]
    print(f"tier 3 built in {time.time() - t0:.1f} s; deciding steps modulo the step block of 16: {sorted(steps)}")
    assert {0, 1, 15} <= steps and time.time() - t0 < 20.0
    # the lift's rows are its own: the double planes' rounding moves them off the planner's rows, by less than the rule allows the device
    for name in P.LIFT_CASES:
        a, b = P._states(P.LIFT + name), P._states(name)
        tl = P.lift_planes(name)[1]
        live = np.arange(a.shape[2])[None, :] < tl[:, None]
        diff = max(float(np.abs(a[:, row] - b[:, row])[live].max()) for row in (3, 4, 5))
        assert 0.0 < diff < 1e-13, (name, diff)
    stop = next(c for c in P.cases(P.LIFT + "scurve_stop_n64") if c.check == "kappa_dot")
    assert (P._rows(P.LIFT + "scurve_stop_n64", stop.j).v == 0).any()      # a standstill carry inside the placed trajectory


def test_planner_velocity_cases_are_decided_and_the_oracle_agrees():
    """tier 3, the velocity check (tests/_kin_plan.py): the slowest pose of each version sits at -1e-5 +- delta with |g| >= 8 B, every
    other margin keeps 1e-6 scale, both deltas come from the oracle and the reference alone, and the double oracle gives the
    reference's status words and counters (delta_small is 64 times what its own error allows the device)."""
    import _kin_plan as P
    import _xref as X
    from oracle import oracle
    for name in P.VELOCITY_CASES:
        v = P.velocity_cases(name)
        assert not P.velocity_not_admitted(v)
        assert [(q[0], q[1]) for q in v.versions] == [("small", 1), ("small", -1), ("large", 1), ("large", -1)]
        assert 8.0 * v.B <= v.small < v.large == K.OTHER * 2e-5 and v.small >= 64 * 8 * v.e_o
        for mask in P.VELOCITY_MASKS:
            for draw in (False, True):
                p, cost, lon, lat, T, tl = P.velocity_plan(name, mask, draw)
                run = oracle.plan_coeffs(p, cost, X.case(name).tables, lon, lat, tl, want_states=False)
                np.testing.assert_array_equal(run.status, v.want[mask, draw])
                np.testing.assert_array_equal(np.asarray(run.out.reason_counts), v.counts[mask, draw])
            fails = S.status_word(2, K.REASON["velocity"], v.step)
            if not v.on_v:      # straight path: above -1e-5 the pose is a standstill with v = 0
                assert list(v.want[mask, True]) == [1, fails] * 2 and list(v.want[mask, False]) == [1, K.REASON["velocity"] << 4] * 2
            else:               # the arc: -1e-5 < v < 0 passes the velocity check and fails the yaw-rate check; the pre-filter sees s_dot
                passes = 1 if mask == K.BIT["velocity"] else S.status_word(2, K.REASON["yaw_rate"], v.step)
                assert list(v.want[mask, True]) == [passes, fails] * 2 and list(v.want[mask, False]) == [K.REASON["velocity"] << 4] * 4
                assert (v.raw[:, v.step] < -1.05e-5).all() and (v.rows[0::2, 3, v.step] > -1e-5).all() and (v.rows[:, 3, v.step] < -0.99e-5).all()
    assert {v % 16 for v, _ in P.VELOCITY_CASES.values()} == {0, 5}
