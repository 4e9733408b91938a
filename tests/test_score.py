"""The scorer (include/rp_score.h, commonroad_rp_amd.trajectory_score) on the device against the draw fixtures and the NumPy
reference of tests/_score.py.  What these tests rest on -- the reference reproduces the fixtures' curvilinear rows, reasons and costs,
it is oracle.frontend.project point by point, and no input pose has a second candidate within 1e-6 m -- is checked on the CPU in
tests/test_score_abi.py.

Shapes: the smallest at which these kernels can go wrong -- a wavefront is 64 consecutive poses of one trajectory, a workgroup four
wavefronts, segment rows are staged in LDS up to a capacity and read from device memory beyond it, and a lane lists up to eight open
segments for itself before its wavefront falls back to walking all segments together."""
import ctypes as C
import math

import numpy as np
import pytest

from commonroad_rp_amd import _capi

import _score as R

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, EABI = -1, -3, -7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same_bits(a, b):
    """Every output of two results equal bit for bit (NaN included)."""
    for name in ("status", "cost", "reason_counts", "s", "d", "theta_cl"):
        np.testing.assert_array_equal(_bits(getattr(a, name)), _bits(getattr(b, name)), err_msg=name)
    assert (a.best, a.n_feasible) == (b.best, b.n_feasible)
    assert a.best_cost == b.best_cost or (math.isnan(a.best_cost) and math.isnan(b.best_cost))


@pytest.fixture(scope="module")
def scorer():
    from commonroad_rp_amd import TrajectoryScorer
    with TrajectoryScorer(0) as sc:
        yield sc


@pytest.fixture(scope="module")
def runs(scorer):
    """Every fixture and every shape once through the device, pruned and exhaustive."""
    out = {}
    for name in R.GPU_FIXTURES:
        f = R.fixture(name)
        scorer.set_reference(f.ref, f.ref_pos, f.ref_theta, f.d_limit)
        out[name] = tuple(scorer.score(f.p, f.cost, want_states=True, flags=fl, **R.fixture_rows(f)) for fl in (0, 1))
    for name in (c[0] for c in R.SHAPES):
        c = R.shape_case(name)
        scorer.set_reference(c.ref, c.ref_pos, c.ref_theta, c.d_limit)
        out[name] = tuple(scorer.score(c.p, c.cost, want_states=True, flags=fl, **R.case_rows(c)) for fl in (0, 1))
    return out


def _against_reference(got, o):
    """s, d, theta_cl to 1e-9 on the valid poses and NaN elsewhere; status words equal; costs to 1e-12 relative; the selection equal."""
    worst = []
    for name in ("s", "d", "theta_cl"):
        g, w = getattr(got, name), getattr(o, name)
        assert g.shape == w.shape and g.dtype == np.float64
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=name)
        fin = ~np.isnan(w)
        worst.append(float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0)
    print(f"largest |device - reference|: s {worst[0]:.1e} m, d {worst[1]:.1e} m, theta_cl {worst[2]:.1e} rad")
    assert max(worst) <= R.TOL
    np.testing.assert_array_equal(got.status, o.status)
    np.testing.assert_array_equal(np.isnan(got.cost), np.isnan(o.cost))
    ok = ~np.isnan(o.cost)
    if ok.any():
        rel = np.abs(got.cost[ok] - o.cost[ok]) / np.abs(o.cost[ok])
        print(f"largest relative cost difference: {rel.max():.1e} over {int(ok.sum())} trajectories")
        assert rel.max() <= R.COST_RTOL
    assert got.best == o.best and got.n_feasible == o.n_feasible
    np.testing.assert_array_equal(got.reason_counts, o.reason_counts)
    if o.best >= 0:
        assert got.best_cost == got.cost[got.best]
    else:
        assert math.isnan(got.best_cost)


# ---- 1. the pins, through the library ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GPU_FIXTURES)
def test_fixture_round_trip_verdicts_costs_and_selection(runs, name):
    f, o, got = R.fixture(name), R.fixture_reference(name), runs[name][0]
    _against_reference(got, o)
    valid = o.valid
    for g, row in ((got.s, R.RP_S), (got.d, R.RP_D), (got.theta_cl, R.RP_THETA_CL)):   # ... and to the fixture itself
        assert np.abs(g - f.states[:, row])[valid].max() <= R.TOL
    np.testing.assert_array_equal(got.reason, f.reason)
    np.testing.assert_array_equal(got.label == 1, f.reason == 0)
    full = (got.status == 1) & (f.lengths == f.n)
    if full.any():
        assert (np.abs(got.cost[full] - f.fixture_cost[full]) / np.abs(f.fixture_cost[full])).max() <= R.COST_RTOL
    if name == "cfg2_ref_draw":
        assert int(full.sum()) == 4


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.SHAPES])
def test_shapes_against_reference(runs, name):
    c = R.shape_case(name)
    assert R.near_ties(c.ref, c.ref_pos, c.x, c.y, c.d_limit) == 0
    _against_reference(runs[name][0], c.ref_out)


@pytest.mark.parametrize("n_points", [1, 64, 65, 1000])
def test_project_points(scorer, n_points):
    c = R.shape_case("n65_k257")
    scorer.set_reference(c.ref, c.ref_pos, c.ref_theta, 2.0)      # a limit that leaves some of the points outside
    x, y = c.x.ravel()[::13][:n_points].copy(), c.y.ravel()[::13][:n_points].copy()
    if n_points > 1:
        x[n_points // 2] = math.nan
    assert R.near_ties(c.ref, c.ref_pos, x, y, 2.0) == 0
    ws, wd, wseg, _ = R.project_batch(c.ref, c.ref_pos, x, y, 2.0)
    s, d, seg, n_outside = scorer.project(x, y, want_outside=True)
    assert s.shape == d.shape == seg.shape == (n_points,) and seg.dtype == np.int32
    np.testing.assert_array_equal(seg, wseg)
    assert n_outside == int((wseg < 0).sum()) and (n_points < 64 or 0 < n_outside < n_points)
    np.testing.assert_array_equal(np.isnan(s), wseg < 0)
    np.testing.assert_array_equal(np.isnan(d), wseg < 0)
    inside = wseg >= 0
    assert np.abs(s[inside] - ws[inside]).max() <= R.TOL and np.abs(d[inside] - wd[inside]).max() <= R.TOL
    s2, d2, seg2 = scorer.project(x.reshape(1, -1), y.reshape(1, -1))                    # the shape of x is kept
    assert s2.shape == (1, n_points) and np.array_equal(_bits(s2.ravel()), _bits(s))


# ---- 3. the tie rule and the domain limit ----------------------------------------------------------------------------------------
def test_tie_rule_and_domain_limit_on_the_u_path(scorer):
    """(4, 2) is at |d| = 2.0 exactly on the first and on the last segment of the U: the first wins, pruned or not -- pruning against a
    held |d| = 2.0 may drop the equal candidate of the LAST segment, never the first."""
    ref, pos, th = R.path("u")
    scorer.set_reference(ref, pos, th, 20.0)
    s, d, seg, n_outside = scorer.project([4.0, 4.0], [2.0, 3.0], want_outside=True)
    assert (s[0], d[0], seg[0]) == (4.0, 2.0, 0) and n_outside == 0
    assert seg[1] == 5 and d[1] == 1.0 and abs(s[1] - (28.0 + 4.0 * math.sqrt(2.0))) <= R.TOL
    f = R.fixture("cfg2_ref_draw")
    rows = dict(x=[[4.0, 4.0]], y=[[2.0, 3.0]], theta=[[0.0, 0.0]], v=np.ones((1, 2)), a=np.zeros((1, 2)), kappa=np.zeros((1, 2)))
    pruned, full = (scorer.score(f.p, f.cost, want_states=True, flags=fl, **rows) for fl in (0, 1))
    _same_bits(pruned, full)
    assert pruned.s[0, 0] == 4.0 and pruned.d[0, 0] == 2.0 and pruned.theta_cl[0, 0] == 0.0
    assert pruned.s[0, 1] == s[1] and abs(pruned.theta_cl[0, 1] + math.pi) <= R.TOL      # heading 0 on a segment that runs at pi
    assert pruned.status[0] == 1
    scorer.set_reference(ref, pos, th, 1.5)
    s, d, seg, n_outside = scorer.project([4.0, 4.0], [2.0, 3.0], want_outside=True)
    assert seg[0] == -1 and math.isnan(s[0]) and math.isnan(d[0]) and n_outside == 1 and seg[1] == 5
    out = scorer.score(f.p, f.cost, want_states=True, **rows)
    assert out.status[0] == R.status_word(2, R.OUT_OF_DOMAIN, 0) and out.reason_counts[6] == 1 and out.best == -1


# ---- 4. pruning ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GPU_FIXTURES) + [c[0] for c in R.SHAPES])
def test_pruned_walk_is_bit_equal_to_the_exhaustive_walk(runs, name):
    _same_bits(*runs[name])


# ---- 5. against rp_project of librp_amd.so ---------------------------------------------------------------------------------------
def test_project_matches_rp_project_point_by_point(scorer):
    checked = outside = 0
    worst = 0.0
    for name in R.GPU_FIXTURES:
        f = R.fixture(name)
        valid = R.fixture_reference(name).valid
        x, y = f.states[:, R.RP_X][valid][::11][:130].copy(), f.states[:, R.RP_Y][valid][::11][:130].copy()
        head = f.ref_theta[0]
        x[::6] -= 19.0 * math.sin(head)                      # every sixth point far to the side: some leave the domain
        y[::6] += 19.0 * math.cos(head)
        d_limit = min(f.d_limit, 18.0)
        scorer.set_reference(f.ref, f.ref_pos, f.ref_theta, d_limit)
        s, d, seg = scorer.project(x, y)
        for q in range(len(x)):
            checked += 1
            try:
                ws, wd = _capi.project(f.ref, f.ref_pos, x[q], y[q], d_limit)
            except ValueError:
                outside += 1
                assert seg[q] == -1 and math.isnan(s[q]), (name, q)
                continue
            assert seg[q] >= 0, (name, q)
            worst = max(worst, abs(s[q] - ws), abs(d[q] - wd))
    print(f"{checked} points, {outside} outside the domain, largest difference {worst:.1e} m")
    assert checked >= 400 and outside >= 5 and worst <= R.TOL


# ---- 6. selection edges ----------------------------------------------------------------------------------------------------------
def _feasible_block(f):
    k = int(np.flatnonzero((R.fixture_reference(f.name).status == 1) & (f.lengths == f.n))[0])
    return {q: r[k].copy() for q, r in R.fixture_rows(f).items() if q != "lengths"}


def test_selection_edges(scorer):
    f = R.fixture("cfg2_ref_draw")
    scorer.set_reference(f.ref, f.ref_pos, f.ref_theta, f.d_limit)
    one = _feasible_block(f)
    n = f.n

    def batch(K):
        return {q: np.tile(r, (K, 1)) for q, r in one.items()}
    # two (here: three) trajectories with bit-equal cost, a more expensive one in front: the smallest k of the equal ones wins
    rows = batch(4)
    rows["a"][0, 3] += 0.5 if rows["a"][0, 3] >= 0.0 else -0.5
    out = scorer.score(f.p, f.cost, **rows)
    assert (out.status == 1).all() and out.cost[1] == out.cost[2] == out.cost[3] < out.cost[0]
    assert out.best == 1 and out.best_cost == out.cost[1] and out.n_feasible == 4 and out.reason_counts.sum() == 0
    # all infeasible
    rows = batch(3)
    rows["a"][:, 7] = 100.0
    out = scorer.score(f.p, f.cost, **rows)
    assert (out.status == R.status_word(2, R.REASON["acceleration"], 7)).all() and np.isnan(out.cost).all()
    assert out.best == -1 and math.isnan(out.best_cost) and out.n_feasible == 0 and out.reason_counts[2] == 3 and out.reason_counts.sum() == 3
    # a NaN pose in the middle of an otherwise feasible trajectory: out of the domain at that step; its neighbours are untouched
    rows = batch(3)
    rows["x"][1, 11] = math.nan
    out = scorer.score(f.p, f.cost, want_states=True, **rows)
    assert out.status[1] == R.status_word(2, R.OUT_OF_DOMAIN, 11) and out.status[0] == out.status[2] == 1
    assert np.isnan(out.s[1, 11]) and not np.isnan(np.delete(out.s[1], 11)).any() and out.best == 0 and out.reason_counts[6] == 1
    # a kinematic failure LATER than a pose outside the domain still decides (the reference runs the whole kinematic loop first)
    rows["kappa"][1, 20:] += 5.0
    out = scorer.score(f.p, f.cost, **rows)
    assert out.status[1] == R.status_word(2, R.REASON["kappa"], 20) and out.reason_counts[3] == 1 and out.reason_counts[6] == 0
    # ... and the order of the checks within a step: velocity before kappa before acceleration
    rows = batch(1)
    rows["a"][0, n - 1] = 100.0
    rows["kappa"][0, n - 1] = 5.0
    assert scorer.score(f.p, f.cost, **rows).status[0] == R.status_word(2, R.REASON["kappa"], n - 1)
    rows["v"][0, n - 1] = -1.0
    assert scorer.score(f.p, f.cost, **rows).status[0] == R.status_word(2, R.REASON["velocity"], n - 1)


def test_rates_across_wavefront_edges(scorer):
    """Yaw rate and kappa_dot of pose 64 and pose 128 read pose 63 and pose 127 -- the last lane of the wavefront before."""
    c = R.shape_case("n130")
    scorer.set_reference(c.ref, c.ref_pos, c.ref_theta, c.d_limit)
    rows = {q: np.tile(r[1], (4, 1)) for q, r in R.case_rows(c).items() if q != "lengths"}      # (all 130 poses of trajectory 1)
    assert (R.reference(c.p, c.cost, c.ref, c.ref_pos, c.ref_theta, **rows).status == 1).all()
    rows["theta"][0, 64:] += 0.6
    rows["theta"][1, 128:] += 0.6
    rows["kappa"][2, 64:] += 0.05
    rows["kappa"][3, 128:] += 0.05
    out = scorer.score(c.p, c.cost, **rows)
    want = R.reference(c.p, c.cost, c.ref, c.ref_pos, c.ref_theta, **rows)
    np.testing.assert_array_equal(out.status, want.status)
    assert list(out.status) == [R.status_word(2, R.REASON["yaw_rate"], 64), R.status_word(2, R.REASON["yaw_rate"], 128),
                                R.status_word(2, R.REASON["kappa_dot"], 64), R.status_word(2, R.REASON["kappa_dot"], 128)]


# ---- 7. lifecycle and arguments --------------------------------------------------------------------------------------------------
def _rc(sc, fn, *args):
    return getattr(sc._lib, fn)(sc._h, *args)


def test_argument_errors():
    from commonroad_rp_amd import TrajectoryScorer
    from commonroad_rp_amd.trajectory_score import _dp, _ip
    f = R.fixture("cfg2_ref_draw")
    one = _feasible_block(f)
    x, y, th, v, a, ka = (np.ascontiguousarray(one[q][None]) for q in ("x", "y", "theta", "v", "a", "kappa"))
    n = f.n
    nul, nuli = C.cast(None, _dp), C.cast(None, _ip)

    def evaluate(sc, p=f.p, cost=f.cost, K=1, n_poses=n, arrays=(x, y, th, v, a, ka), lens=None, flags=0):
        ptr = [nul if q is None else _capi.dptr(q) for q in arrays]
        return _rc(sc, "rp_score_evaluate", C.byref(p), C.byref(cost), K, n_poses, *ptr, nuli if lens is None else lens.ctypes.data_as(_ip), flags,
                   nul, nul, nul, None, nul, None, nul, None, None)
    with TrajectoryScorer(0) as sc:
        # no reference yet
        assert evaluate(sc) == ESTATE and b"reference" in sc._lib.rp_score_last_error(sc._h)
        assert _rc(sc, "rp_score_project", 1, _capi.dptr(x), _capi.dptr(y), nul, nul, nuli, None) == ESTATE
        # set_reference
        ref, pos, theta = f.ref, f.ref_pos, f.ref_theta

        def set_ref(n_v=len(pos), r=ref, p=pos, t=theta, lim=20.0):
            return _rc(sc, "rp_score_set_reference", n_v, _capi.dptr(_capi.f64(r)), _capi.dptr(_capi.f64(p)), _capi.dptr(_capi.f64(t)), lim)
        bad_pos, bad_xy, nan_th, flat = pos.copy(), ref.copy(), theta.copy(), pos.copy()
        bad_pos[5] = bad_pos[4]
        bad_xy[9] = bad_xy[8]
        nan_th[3] = math.nan
        flat[7] = math.inf
        for kw in (dict(n_v=1), dict(p=bad_pos), dict(r=bad_xy), dict(t=nan_th), dict(p=flat), dict(lim=0.0), dict(lim=-1.0), dict(lim=math.nan)):
            assert set_ref(**kw) == EINVAL, kw
        assert evaluate(sc) == ESTATE                     # ... and a refused table is no table
        assert set_ref() == 0
        assert evaluate(sc) == 0
        # evaluate
        assert evaluate(sc, K=-1) == EINVAL and evaluate(sc, n_poses=0) == EINVAL
        assert evaluate(sc, K=(1 << 24) + 1, n_poses=1) == EINVAL and evaluate(sc, K=1 << 20, n_poses=17) == EINVAL
        for lens in ([0], [n + 1], [-3]):
            assert evaluate(sc, lens=np.array(lens, dtype=np.int32)) == EINVAL
        assert evaluate(sc, lens=np.array([n], dtype=np.int32)) == 0
        for missing in (0, 1, 2):
            arrays = [x, y, th, v, a, ka]
            arrays[missing] = None
            assert evaluate(sc, arrays=arrays) == EINVAL
        assert evaluate(sc, arrays=(x, y, th, None, a, ka)) == EINVAL            # the mask asks for the velocity check
        assert evaluate(sc, arrays=(x, y, th, v, a, None)) == EINVAL             # ... and for kappa
        assert evaluate(sc, arrays=(x, y, th, v, None, ka)) == EINVAL            # a: the acceleration check and the cost
        relaxed = _capi.copy_params(f.p)
        relaxed.constraint_mask = 0
        assert evaluate(sc, p=relaxed, arrays=(x, y, th, v, None, ka)) == EINVAL   # the cost's acceleration term alone
        assert evaluate(sc, p=relaxed, arrays=(x, y, th, None, a, None)) == EINVAL  # desired_speed is set: v
        no_speed = _capi.make_cost(desired_speed=None)
        assert evaluate(sc, p=relaxed, cost=no_speed, arrays=(x, y, th, None, a, None)) == 0
        assert evaluate(sc, p=relaxed, cost=_capi.make_cost(kind=1), arrays=(x, y, th, None, a, None)) == 0
        assert evaluate(sc, cost=_capi.make_cost(kind=2)) == EINVAL              # RP_COST_EXTERNAL
        for kw in (dict(desired_speed=math.inf), dict(desired_d=-math.inf), dict(desired_s=math.inf)):
            assert evaluate(sc, cost=_capi.make_cost(**kw)) == EINVAL, kw
        assert evaluate(sc, flags=2) == EINVAL
        short = _capi.copy_params(f.p)
        short.struct_size -= 8
        assert evaluate(sc, p=short) == EABI
        small = _capi.make_cost()
        small.struct_size -= 8
        assert evaluate(sc, cost=small) == EABI
        # project
        assert _rc(sc, "rp_score_project", -1, _capi.dptr(x), _capi.dptr(y), nul, nul, nuli, None) == EINVAL
        assert _rc(sc, "rp_score_project", 3, nul, _capi.dptr(y), nul, nul, nuli, None) == EINVAL
        assert _rc(sc, "rp_score_project", (1 << 24) + 1, _capi.dptr(x), _capi.dptr(y), nul, nul, nuli, None) == EINVAL
        n_out = C.c_int64(7)
        assert _rc(sc, "rp_score_project", 0, nul, nul, nul, nul, nuli, C.byref(n_out)) == 0 and n_out.value == 0
        # K == 0
        out = sc.score(f.p, f.cost, np.empty((0, n)), np.empty((0, n)), np.empty((0, n)), v=np.empty((0, n)), a=np.empty((0, n)), kappa=np.empty((0, n)))
        assert out.best == -1 and math.isnan(out.best_cost) and out.n_feasible == 0 and not out.reason_counts.any() and out.status.shape == (0,)
        with pytest.raises(_capi.RpError, match="-1"):
            sc.score(f.p, _capi.make_cost(kind=2), x, y, th, v=v, a=a, kappa=ka)


def test_second_reference_replaces_the_first_and_results_do_not_depend_on_the_call_before():
    from commonroad_rp_amd import TrajectoryScorer
    big, small, fx = R.shape_case("n65_k257"), R.shape_case("n64_ragged"), R.fixture("cfg2_ref_draw")
    with TrajectoryScorer(0) as fresh:
        fresh.set_reference(small.ref, small.ref_pos, small.ref_theta, small.d_limit)
        want = fresh.score(small.p, small.cost, want_states=True, **R.case_rows(small))
    with TrajectoryScorer(0) as sc:
        sc.set_reference(big.ref, big.ref_pos, big.ref_theta, big.d_limit)           # another path first, and a large K
        first = sc.score(big.p, big.cost, want_states=True, **R.case_rows(big))
        assert first.n_feasible == big.ref_out.n_feasible
        sc.set_reference(small.ref, small.ref_pos, small.ref_theta, small.d_limit)   # the second table is the one used
        _same_bits(sc.score(small.p, small.cost, want_states=True, **R.case_rows(small)), want)
        # NULL outputs in every combination the binding uses: no states; and the C entry with one state plane at a time
        bare = sc.score(small.p, small.cost, **R.case_rows(small))
        assert bare.s is None and bare.d is None and bare.theta_cl is None
        np.testing.assert_array_equal(bare.status, want.status)
        np.testing.assert_array_equal(_bits(bare.cost), _bits(want.cost))
        assert (bare.best, bare.n_feasible) == (want.best, want.n_feasible)
        from commonroad_rp_amd.trajectory_score import _dp, _ip
        rows = {q: np.ascontiguousarray(r) for q, r in R.case_rows(small).items()}
        K, n = rows["x"].shape
        nul = C.cast(None, _dp)
        for which in range(3):
            buf = np.full((K, n), 7.0)
            outs = [nul, nul, nul]
            outs[which] = _capi.dptr(buf)
            rc = sc._lib.rp_score_evaluate(sc._h, C.byref(small.p), C.byref(small.cost), K, n, *(_capi.dptr(rows[q]) for q in ("x", "y", "theta", "v", "a", "kappa")),
                                           rows["lengths"].ctypes.data_as(_ip), 0, *outs, None, nul, None, nul, None, None)
            assert rc == 0
            np.testing.assert_array_equal(_bits(buf), _bits((want.s, want.d, want.theta_cl)[which]))
    del fx


def test_score_states_on_a_live_plan_equals_score_on_its_rows(scorer):
    """The [C, RP_N_ARRAYS, N + 1] blocks of fetch_states() of a small draw-mode plan, each over its own length."""
    from _golden import Golden
    from commonroad_rp_amd._capi import RpContext
    g = Golden("arc_hv_l1_draw")
    ctx = RpContext(0)
    try:
        g.setup_context(ctx)
        g.inputs.params.flags |= _capi.FLAG_MATERIALIZE_ALL
        ctx.plan(g.inputs)
        states = ctx.fetch_states()
        status, _ = ctx.fetch_status()
    finally:
        ctx.close()
    nLD = len(g["L"]) * len(g["D"])
    lengths = np.repeat(g["traj_len"], nLD).astype(np.int32)
    assert states.shape == (len(lengths), 14, int(g["N"]) + 1)
    pick = np.arange(0, len(lengths), 3)
    scorer.set_reference(g["ref_path"], g["ref_pos"], g["ref_theta"], float(g["proj_d_limit"]))
    p, cost = g.inputs.params, g.inputs.cost
    a = scorer.score_states(p, cost, states[pick], lengths=lengths[pick], want_states=True)
    st = states[pick]
    b = scorer.score(p, cost, st[:, 0], st[:, 1], st[:, 2], v=st[:, 3], a=st[:, 4], kappa=st[:, 5], lengths=lengths[pick], want_states=True)
    _same_bits(a, b)
    # the plan's own kinematic verdicts on those candidates (its collision label aside), and its curvilinear rows on their own lengths
    np.testing.assert_array_equal(a.reason, (status[pick] >> 4) & 7)
    valid = np.arange(st.shape[2])[None, :] < lengths[pick][:, None]
    for got, row in ((a.s, R.RP_S), (a.d, R.RP_D), (a.theta_cl, R.RP_THETA_CL)):
        assert np.abs(got - st[:, row])[valid].max() <= R.TOL
    with pytest.raises(ValueError):
        scorer.score_states(p, cost, states[0])
