"""Kinematic verdicts of the HIP paths at their thresholds against the exact reference of tests/_kin.py: label, reason and first
failing step of trajectories whose one placed margin sits 64 B = 1024 u scale, 2^16 B or 1e-6 scale on either side of a bound of
``_check_constraints`` -- or on the bound itself and the doubles beside it where no rounding is involved -- with the deciding step
on the first, second and last lane of a wavefront and on a trajectory's last pose, under the full mask, the mask of each check alone,
the full mask without each check and every pair of checks.  The reference decides every case (tests/test_kin_abi.py); a verdict here
is right or wrong, there is no tolerance.

Tier 1: rp_score_evaluate, whose checked quantities are its inputs (two vehicles: for the second, libm's and NumPy's tangent of
delta_max differ by an ulp).  Tier 2: rp_lift_evaluate on a straight path in low-velocity mode with d_dot = 0, where v, a and kappa
are copies of s_dot, s_ddot and d_ddot: the families of velocity, acceleration, kappa and kappa_dot through the lift's own
step_reason and its carry from one chunk of 64 poses to the next; its input branch edges; and, with the vehicle limit placed against
quantities the lift computes itself on curved paths, tests/_kin_plan.py.  Tier 3: the planner's kernels through rp_plan on nine launch
paths in production and draw mode, the vehicle limit placed against the extended-precision rows of tests/_xref.py; the bound itself
for kappa; and the velocity check through rp_plan_coeffs, a coefficient of an explicit polynomial placed."""
import numpy as np
import pytest

import _kin as K
import _kin_plan as P
import _lift
import _score as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not K.HAVE_LONGDOUBLE, reason=K.SKIP_REASON)]

MASK_SETS = {"full": K.MASKS[:1], "one_check": K.MASKS[1:6], "one_check_cleared": K.MASKS[6:11], "pairs": K.MASKS[11:]}


def _wrong(g, got, want):
    return [(int(k), str(g.family[k]), g.rows[k].level, int(g.rows[k].sign), f"got {int(got[k]):#x}", f"want {int(want[k]):#x}")
            for k in np.flatnonzero(got != want)[:12]]


@pytest.fixture(scope="module")
def scorer_runs():
    """Every vehicle under every mask, once"""
    from commonroad_rp_amd import TrajectoryScorer
    ref, pos, th = S.path("two_vertex")
    out = {}
    with TrajectoryScorer(0) as sc:
        sc.set_reference(ref, pos, th, 20.0)
        for name in K.vehicles():
            g = K.group(name)
            for m in K.MASKS:
                out[name, m] = K.device_scorer(sc, g, m)
    return out


@pytest.mark.parametrize("masks", list(MASK_SETS))
@pytest.mark.parametrize("name", list(K.vehicles()))
def test_scorer_verdicts_counts_and_selection(scorer_runs, name, masks):
    g = K.group(name)
    for m in MASK_SETS[masks]:
        got, want = scorer_runs[name, m], g.want[m]
        bad = _wrong(g, got.status, want)
        print(f"{name} mask {m:2d}: {len(want)} trajectories, {int((want == 1).sum())} feasible, {len(bad)} differ")
        assert not bad, (m, bad)
        best, n_feasible, counts = K.selection(g, m)
        assert got.n_feasible == n_feasible and got.best == best
        np.testing.assert_array_equal(got.reason_counts, counts)
        assert np.isnan(got.cost[want != 1]).all()


def test_scorer_own_check_alone_on_every_placed_case(scorer_runs):
    """What the table of a family reads as: "+" feasible, "-" its own reason at its own step, under the mask of that check alone;
    feasible with the bit cleared wherever nothing else is wrong with the row."""
    seen = set()
    for name in K.vehicles():
        g = K.group(name)
        for k, r in enumerate(g.rows):
            c = K.own_check(r)
            if c is None:
                continue
            st = int(scorer_runs[name, K.BIT[c]].status[k])
            assert st == (1 if r.sign > 0 else S.status_word(2, K.REASON[c], int(r.step))), (name, k, r.family, r.level, r.sign, hex(st))
            cleared = int(scorer_runs[name, K.FULL & ~K.BIT[c]].status[k])
            assert cleared == int(g.want[K.FULL & ~K.BIT[c]][k]) and (cleared >> 4) & 7 != K.REASON[c]
            seen.add((r.family, r.sign, int(r.step) % 64))
    assert {(f, s) for f, s, _ in seen} >= {(f, s) for f in ("kappa", "acc_switch", "kappa_dot", "yaw_bound", "yaw_half", "yaw_tie") for s in (1, -1)}
    assert {lane for _, _, lane in seen} >= {0, 1, 63}


# ---- tier 2: the lift --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lift_runs():
    from commonroad_rp_amd.lift import TrajectoryLifter
    g = K.group("std", lift=True)
    with TrajectoryLifter(0) as lf:
        lf.set_reference(*_lift.table_args(_lift.built_path(K.LIFT_POINTS)))
        return {m: lf.lift(K.lift_params(g.veh, m), **K.lift_inputs(g, K.lift_raw_v())) for m in K.LIFT_MASKS}


def test_lift_rows_are_copies_of_its_inputs(lift_runs):
    """What exact placement rests on: straight path, low-velocity mode, d_dot = 0"""
    g, r = K.group("std", lift=True), lift_runs[K.FULL]
    live = np.arange(K.N_POSES)[None, :] < g.lengths[:, None]
    for got, want in ((r.v, g.v), (r.a, g.a), (r.kappa, g.kappa)):
        assert np.array_equal(got[live], want[live])
    assert np.ptp(r.theta[live]) == 0.0 and np.isnan(r.v[~live]).all()


@pytest.mark.parametrize("masks", ["full", "one_check", "one_check_cleared"])
def test_lift_verdicts_and_counts(lift_runs, masks):
    g = K.group("std", lift=True)
    for m in MASK_SETS[masks]:
        got, want = lift_runs[m], g.want[m]
        bad = _wrong(g, got.status, want)
        print(f"lift mask {m:2d}: {len(want)} trajectories, {int((want == 1).sum())} feasible, {len(bad)} differ")
        assert not bad, (m, bad)
        feasible = np.flatnonzero(want == 1)
        assert got.n_feasible == feasible.size and got.first_feasible == (int(feasible[0]) if feasible.size else -1)
        np.testing.assert_array_equal(got.reason_counts, np.bincount((want[want != 1] >> 4) & 7, minlength=8))
    deciding = {int(r.step) for r in g.rows if r.sign < 0}
    assert {63, 64, 65, 128} <= deciding


def test_lift_input_branch_edges():
    """s_dot at +-1e-5 and 0.001, d_dot at +-1e-5 and the doubles beside them, from poses 1, 63, 64 and 65 on (63: the standstill carry
    starts on the last lane of a chunk): rows to the tolerances of tests/test_lift.py, verdicts and reductions equal."""
    from commonroad_rp_amd.lift import TrajectoryLifter
    c = K.lift_edges()
    o = c.out
    with TrajectoryLifter(0) as lf:
        lf.set_reference(*_lift.table_args(c.path))
        got = lf.lift(c.p, lengths=c.lengths, **c.planes)
    for name in _lift.PLANES:
        g, w = getattr(got, name), getattr(o, name)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=name)
        fin = ~np.isnan(w)
        worst = float(np.abs(g[fin] - w[fin]).max())
        print(f"{name}: largest |device - reference| {worst:.1e}")
        assert worst <= (_lift.TOL if name in ("x", "y", "theta", "theta_cl") else _lift.STATE_ATOL), name
    zero = o.v == 0.0
    assert zero.any() and (got.v[zero] == 0.0).all()          # a speed the input rule zeroes is zero, not small
    kept = np.zeros_like(zero)
    kept[:, 1:] = (o.theta[:, 1:] == o.theta[:, :-1])
    assert kept.any() and (got.theta[:, 1:][kept[:, 1:]] == got.theta[:, :-1][kept[:, 1:]]).all()   # an orientation that is kept is a copy
    bad = [(int(k), c.what[k], hex(int(got.status[k])), hex(int(o.status[k]))) for k in np.flatnonzero(got.status != o.status)]
    assert not bad, bad[:10]
    assert (got.first_feasible, got.n_feasible) == (o.first_feasible, o.n_feasible)
    np.testing.assert_array_equal(got.reason_counts, o.reason_counts)


# ---- tier 3: the planner's kernels, the vehicle limit placed against the extended-precision rows (tests/_kin_plan.py) --------------
@pytest.fixture(scope="module")
def plan_contexts():
    """one context per launch path, made when first asked for"""
    from commonroad_rp_amd._capi import RpContext
    from _paths import LAUNCH_PATHS
    made = {}

    def get(path):
        if path not in made:
            made[path] = RpContext(0)
            for k, v in LAUNCH_PATHS[path].items():
                made[path].set_option(k, v)
        return made[path]
    yield get
    for ctx in made.values():
        ctx.close()


def _production_kernel(path, N):
    """the kernel a production-mode plan without a collision query takes on a launch path (tests/_paths.py, as tests/test_xref.py)"""
    from _bitid import chunk_applies
    if path == "lane_cand":
        return "rp_cost_kernel"
    if path == "lane_chunk" and chunk_applies(N):
        return "rp_chunk_kernel"
    return "rp_eval_kernel"


@pytest.mark.parametrize("name", P.CASES)
@pytest.mark.parametrize("path", list(P.LAUNCH_PATHS))
def test_planner_verdicts_at_placed_limits(plan_contexts, path, name):
    """a_max, delta_max or v_delta_max set delta_small and delta_large on either side of what the binding step of one candidate needs,
    and two limits halved at once (priority): label, reason and first failing step of that candidate in production and in draw mode,
    on the kernel the launch path stands for"""
    import _xref as XR
    from commonroad_rp_amd.collision import ObstacleTables
    ctx = plan_contexts(path)
    c0 = XR.case(name)
    ctx.set_coordinate_system(c0.co)
    ctx.set_obstacles(ObstacleTables())
    cases = P.cases(name)
    assert {c.check for c in cases} == set(P.LIMIT) | {"priority"}
    bad, kernels = [], set()
    for c in cases:
        for draw in (False, True):
            out = ctx.plan(P.plan_inputs(name, c, draw))
            kernels.add((draw, ctx.last_kernel()))
            assert ctx.last_kernel() == ("rp_eval_kernel" if draw else _production_kernel(path, c0.inp.params.N)), (path, draw, ctx.last_kernel())
            if "lanes" in P.LAUNCH_PATHS[path] and ctx.last_kernel() == "rp_eval_kernel":
                assert ctx.get_option("last_lanes") == P.LAUNCH_PATHS[path]["lanes"]
            if P.LAUNCH_PATHS[path].get("fused_lon", 1) == 0:
                assert ctx.get_option("last_single_launch") == 0
            st, _ = ctx.fetch_status()
            got, want = int(st[c.index]), int(c.want[draw])
            if got != want:
                bad.append((c.check, c.level, c.sign, "draw" if draw else "production", f"candidate {c.index} step {c.step}", f"got {got:#x}", f"want {want:#x}"))
            elif (want & 3) == 2:
                assert out.reason_counts[(want >> 4) & 7] >= 1
    print(f"{name} on {path}: {2 * len(cases)} plans, kernels {sorted(kernels)}, {len(bad)} verdicts differ")
    assert not bad, bad


# ---- tier 2, derived quantities: the lift's own v, a, kappa and theta on curved paths, the vehicle limit placed -------------------------
@pytest.mark.parametrize("name", P.LIFT_CASES)
def test_lift_verdicts_at_placed_limits(name):
    """The candidates of a case as given trajectories (their curvilinear planes rounded to doubles; |d| up to 4 m on the 25 m arc, a
    standstill carry in the stopping case): the lift's formulas are evaluated in double-word arithmetic on those doubles, the limit is
    placed against the binding step of one of them, and the lift's verdict on that trajectory is the reference's."""
    import _xref as XR
    from commonroad_rp_amd.lift import TrajectoryLifter
    cases = P.cases(P.LIFT + name)
    assert {c.check for c in cases} == set(P.LIMIT) | {"priority"}
    bad = []
    with TrajectoryLifter(0) as lf:
        lf.set_reference(XR.case(name).co)
        for c in cases:
            p, kw = P.lift_call(name, c)
            got, want = int(lf.lift(p, **kw).status[c.j]), int(c.want[True])
            if got != want:
                bad.append((c.check, c.level, c.sign, f"candidate {c.index} step {c.step}", f"got {got:#x}", f"want {want:#x}"))
    print(f"lift on {name}: {len(cases)} calls, {len(bad)} verdicts differ")
    assert not bad, bad


# ---- tier 3, the bound itself: |kappa| == kappa_max passes (">"), the double below it fails -- no rounding, no guard ------------------------
ROWS_OF_PATH = {"single_launch": "default", "g32": "two_kernel_32", "g64": "two_kernel_64"}   # the others: 16 lanes, two kernels


def _delta_for(kmax, wheelbase):
    """(delta_max whose kappa_max, tan(delta_max) / wheelbase in the host's double arithmetic, IS kmax; the largest whose kappa_max is
    below it) -- or None where the two roundings skip kmax"""
    import math
    d = math.atan(wheelbase * kmax)
    for _ in range(64):
        d = np.nextafter(d, 4.0)
    hit = None
    for _ in range(160):
        km = math.tan(d) / wheelbase
        if km == kmax and hit is None:
            hit = float(d)
        if km < kmax:
            return (hit, float(d)) if hit is not None else None
        d = np.nextafter(d, 0.0)
    return None


@pytest.mark.parametrize("path", list(P.LAUNCH_PATHS))
def test_planner_kappa_on_its_bound_passes(plan_contexts, path):
    """The largest |kappa| the device itself stores for a candidate, as kappa_max: the comparison is one of two doubles, the bound
    passes and the next kappa_max below fails at that step.  (What a displaced case cannot see: ">=" for ">".)"""
    import _xref as XR
    from commonroad_rp_amd._capi import RpContext, PlanInputs, copy_params, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL
    from commonroad_rp_amd.collision import ObstacleTables
    # The stored kappa is read on the launch variant of tests/_xref.py that stores rows with this path's lanes per candidate; for the six
    # 16-lane two-kernel paths that is "two_kernel_16", and rp_cost_kernel / rp_chunk_kernel are held to its bits by
    # tests/test_kernel_bit_identity.py (a kappa that differed in its last bit would fail here as well: the bound is that double).
    variant = ROWS_OF_PATH.get(path, "two_kernel_16")
    done = 0
    for name in ("arc_keep_n17", "arc_low_n65", "scurve_stop_n64"):
        c0 = XR.case(name)
        rows_ctx = RpContext(0)
        try:
            states, _ = XR.device_rows(rows_ctx, name, variant)
        finally:
            rows_ctx.close()
        ctx = plan_contexts(path)
        ctx.set_coordinate_system(c0.co)
        ctx.set_obstacles(ObstacleTables())
        for c in [q for q in P.cases(name) if q.check == "kappa" and q.sign > 0 and q.level == "small"]:
            kap = np.abs(states[c.j, XR.KAPPA, :c.tl])
            step, kmax = int(kap.argmax()), float(kap.max())
            found = _delta_for(kmax, float(c0.inp.params.wheelbase))
            if found is None or (np.sort(kap)[-2] == kmax):
                continue
            for delta_max, want in ((found[0], 1), (found[1], S.status_word(2, K.REASON["kappa"], step))):
                for draw in (False, True):
                    p = copy_params(c0.inp.params)
                    p.delta_max, p.constraint_mask = delta_max, K.BIT["kappa"]
                    p.flags = (p.flags & ~(FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)) | (FLAG_DRAW_ALL if draw else 0)
                    ctx.plan(PlanInputs(p, c0.inp.cost, c0.inp.T, c0.inp.traj_len, c0.inp.L, c0.inp.D))
                    assert ctx.last_kernel() == ("rp_eval_kernel" if draw else _production_kernel(path, c0.inp.params.N))
                    got = int(ctx.fetch_status()[0][c.index])
                    assert got == want, (name, path, "draw" if draw else "production", c.index, step, hex(got), hex(want))
            done += 1
    print(f"{path}: {done} candidates whose largest |kappa| is a kappa_max the host can form")
    assert done >= 1     # (tan(delta_max) / wheelbase reaches 173 of 200 random doubles: three candidates to find one among)


# ---- tier 3, the velocity check: explicit polynomials whose slowest pose sits at -1e-5 +- delta (rp_plan_coeffs) ---------------------------
@pytest.mark.parametrize("name", list(P.VELOCITY_CASES))
@pytest.mark.parametrize("path", list(P.LAUNCH_PATHS))
def test_planner_velocity_at_its_threshold(plan_contexts, path, name):
    """The four versions of a case (delta_small, delta_large, above and below -1e-5) as the four candidates of one call, under the
    full mask and the velocity check alone, in production and in draw mode: status words, n_feasible and the reason counters, all of
    which the reference fixes here."""
    import _xref as XR
    from commonroad_rp_amd.collision import ObstacleTables
    ctx = plan_contexts(path)
    c0 = XR.case(name)
    ctx.set_coordinate_system(c0.co)
    ctx.set_obstacles(ObstacleTables())
    v = P.velocity_cases(name)
    kernels = set()
    for mask in P.VELOCITY_MASKS:
        for draw in (False, True):
            out = ctx.plan_coeffs(*P.velocity_plan(name, mask, draw))
            kernels.add((draw, ctx.last_kernel()))
            # (explicit polynomials are always evaluated by rp_eval_kernel: the one-lane kernels serve sampled batches only, rp_host.hip
            #  lane_kernel_ok; what a launch path still varies is one launch or two, the lanes per candidate and the workgroup shape)
            assert ctx.last_kernel() == "rp_eval_kernel", (path, draw, ctx.last_kernel())
            if "lanes" in P.LAUNCH_PATHS[path]:
                assert ctx.get_option("last_lanes") == P.LAUNCH_PATHS[path]["lanes"]
            if P.LAUNCH_PATHS[path].get("fused_lon", 1) == 0:
                assert ctx.get_option("last_single_launch") == 0
            st, _ = ctx.fetch_status()
            want = v.want[mask, draw]
            assert list(st) == list(want), (name, path, mask, "draw" if draw else "production", [hex(int(q)) for q in st], [hex(int(q)) for q in want])
            np.testing.assert_array_equal(np.asarray(out.reason_counts), v.counts[mask, draw])
            assert out.n_feasible == int((want == 1).sum())
    print(f"{name} on {path}: kernels {sorted(kernels)}, step {v.step}, placed v + 1e-5 {[f'{q[3]:+.2e}' for q in v.versions]}")
