"""The pick under a risk bound (include/rp_epick.h, commonroad_rp_amd.ensemble_pick) on the device against the yardstick of
tests/_epick.py and against its siblings on the same device: with one member it is rp_pick_select bit for bit, its planes and kinematic
words are rp_lift_evaluate's, its per-member first hits rp_ensemble_check's.  What these tests rest on -- no first hit of a case moves
when the vehicle grows or shrinks by 2e-6 m, no rival's cost lies within 1e-9 (relative) of a winner's at any bound, the order of the
risk's sum shows in the weights used -- is checked on the CPU in tests/test_epick_abi.py.  Tolerances are those of tests/test_pick.py.

Shapes: the smallest at which these kernels can go wrong -- (trajectory, chunk) wavefronts x blocks of EP_MEMBER_BLOCK members, 64
trajectories per workgroup and 64 members per tile in the risk stage, LDS and device-memory variants for segment rows and static rows.

  every case of tests/_pick.py and its pin, one member     equal to rp_pick_select (K up to 1100: two passes of the final workgroup)
  long_path_m5 16 x 31, M = 5                               a member block and one member more; EP_LF_LDS_ROWS + 1 segments
  factor3_m3 8 x 30, M = 3                                  one member less than a block; time indices on both sides of the tables
  ragged_m9 37 x 65, M = 9                                  two chunks, poses beyond len, a partial workgroup, static hits
  long_path_m65 16 x 31, M = 65                             two member tiles of the risk stage
  boundary 4 x 80, M = two member blocks                    first hits at poses 63 and 64 across members, a segment's own time index,
                                                            the first and the last member of a block
"""
import ctypes as C
import math

import numpy as np
import pytest

from commonroad_rp_amd import _capi
from commonroad_rp_amd.collision import ObstacleTables

import _epick as EP
import _lift as L
import _pick as P
import _score as S
from test_pick import TIGHT

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, EABI = -1, -3, -7
SCALARS = ("best", "best_cost", "n_feasible", "n_collision", "n_collision_before_best", "best_members_hit", "best_risk")
PER_TRAJECTORY = ("status", "cost", "members_hit", "risk", "first_pose_hit", "first_segment_hit")
UNBOUND = ("cost", "members_hit", "risk", "first_pose_hit", "first_segment_hit") + L.PLANES   # what does not depend on the bound


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b, what="", names=PER_TRAJECTORY + ("reason_counts", "best_states") + L.PLANES, scalars=SCALARS):
    """Every output two results both hold equal bit for bit (NaN included)."""
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        if name == "best_states":
            assert (x is None) == (y is None), what
        if x is None or y is None:   # (planes and hit matrices a call did not ask for)
            continue
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{what}: {name}")
    for name in scalars:
        x, y = getattr(a, name), getattr(b, name)
        assert x == y or (x != x and y != y), (what, name, x, y)


@pytest.fixture(scope="module")
def picker():
    from commonroad_rp_amd import EnsemblePicker
    with EnsemblePicker(0) as ep:
        yield ep


def _load(ep, c, weights=None):
    ep.set_reference(*L.table_args(c.path))
    ep.set_static(c.obs)
    ep.set_members(c.members, c.dyn_t0, weights)


def _pick(ep, c, max_risk=0.0, want_planes=True, want_hits=True):
    return ep.pick(c.p, c.cost, *c.planes, lengths=c.lengths, theta0=c.theta0, poses=bool(c.mode & EP.POSES), swept=bool(c.mode & EP.SWEPT),
                   max_risk=max_risk, want_planes=want_planes, want_hits=want_hits)


def _run(ep, c, weights=None, max_risk=0.0, want_planes=True, want_hits=True):
    _load(ep, c, weights)
    return _pick(ep, c, max_risk, want_planes, want_hits)


def _decision_is(got, r, what):
    """Labels, the winner, the counts and the winner's two: EQUAL to the yardstick's"""
    np.testing.assert_array_equal(got.status, r.status, err_msg=what)
    np.testing.assert_array_equal(got.label, r.status & 3)
    np.testing.assert_array_equal(got.reason, (r.status >> 4) & 7)
    np.testing.assert_array_equal(got.step, (r.status >> 8) & 0xFFF)
    assert (got.best, got.n_feasible, got.n_collision, got.n_collision_before_best, got.best_members_hit) == \
        (r.best, r.n_feasible, r.n_collision, r.n_collision_before_best, r.best_members_hit), what
    np.testing.assert_array_equal(got.reason_counts, r.reason_counts, err_msg=what)
    if r.best < 0:
        assert got.best_states is None and np.isnan(got.best_cost) and np.isnan(got.best_risk), what
    else:
        assert _bits(np.float64(got.best_risk)) == _bits(np.float64(r.best_risk)), what
        assert _bits(np.float64(got.best_cost)) == _bits(got.cost[got.best]), what


def _against_reference(got, c, r):
    """The NaN pattern equal and the eight planes to the lift's tolerances; status, members_hit, both hit matrices and every integer
    scalar EQUAL to the yardstick's, the risk bit-equal to it; the cost within COST_RTOL of the cost function applied to the device's
    own planes of the same call; the winner's block bit-equal to the planes and the inputs."""
    o, what = r.lift, c.name
    K, n = c.planes[0].shape
    worst = {}
    for name in L.PLANES:
        g, w = getattr(got, name), getattr(o, name)
        assert g.shape == w.shape == (K, n) and g.dtype == np.float64
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: NaN pattern of {name}")
        fin = ~np.isnan(w)
        worst[name] = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
    print(f"{what}: largest |device - reference| " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= (L.TOL if name in TIGHT else L.STATE_ATOL), (what, name, v)
    _decision_is(got, r, what)
    assert got.members_hit.dtype == np.int32 and got.risk.dtype == np.float64
    np.testing.assert_array_equal(got.members_hit, r.members_hit, err_msg=what)
    np.testing.assert_array_equal(_bits(got.risk), _bits(r.risk), err_msg=what)
    for name, bit in (("first_pose_hit", EP.POSES), ("first_segment_hit", EP.SWEPT)):
        if c.mode & bit:
            assert getattr(got, name).dtype == np.int32 and getattr(got, name).shape == (K, c.M)
            np.testing.assert_array_equal(getattr(got, name), getattr(r, name), err_msg=f"{what}: {name}")
        else:
            assert getattr(got, name) is None
    feasible = (r.status & 3) != 2
    np.testing.assert_array_equal(np.isnan(got.cost), ~feasible, err_msg=what)
    worst_cost = 0.0
    for k in np.flatnonzero(feasible):
        m = int(o.lengths[k])
        want = S.cost_of(c.cost, got.a[k, :m], got.v[k, :m], c.planes[0][k, :m], c.planes[3][k, :m], got.theta_cl[k, :m])
        worst_cost = max(worst_cost, abs(got.cost[k] - want) / want)
    print(f"{what}: largest relative |cost - cost_of(device planes)| {worst_cost:.1e} over {int(feasible.sum())} trajectories")
    assert worst_cost <= S.COST_RTOL, what
    if r.best < 0:
        return
    m = int(o.lengths[r.best])
    block = got.best_states
    assert block.shape == (14, n)
    for row, name in zip(P.PLANE_ROWS, L.PLANES):
        np.testing.assert_array_equal(_bits(block[row]), _bits(getattr(got, name)[r.best]), err_msg=f"{what}: row {row} of the winner's block")
    for row, q in zip(P.INPUT_ROWS, c.planes):
        np.testing.assert_array_equal(_bits(block[row, :m]), _bits(q[r.best, :m]), err_msg=f"{what}: row {row} of the winner's block")
        assert np.isnan(block[row, m:]).all()


def _case(name):
    return EP.boundary() if name == "boundary" else EP.multi(name)


# ---- 1. one member is the pick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pin"] + list(P.CASES))
def test_one_member_equals_the_pick(picker, name):
    """One member, NULL weights, max_risk 0: every output bit-equal to rp_pick_select's on the same tables in the same process."""
    from commonroad_rp_amd import TrajectoryPicker
    c = EP.single(name)
    got = _run(picker, c)
    with TrajectoryPicker(0) as pk:
        pk.set_reference(*L.table_args(c.path))
        pk.set_obstacles(c.obs)
        want = pk.pick(c.p, c.cost, *c.planes, lengths=c.lengths, theta0=c.theta0, poses=bool(c.mode & EP.POSES), swept=bool(c.mode & EP.SWEPT),
                       want_planes=True, want_hits=True)
    _same_bits(got, want, name, names=("status", "cost", "reason_counts", "best_states") + L.PLANES, scalars=SCALARS[:5])
    K = len(want.status)
    for attr in ("first_pose_hit", "first_segment_hit"):
        g, w = getattr(got, attr), getattr(want, attr)
        assert (g is None) == (w is None), attr
        if w is not None:
            assert g.shape == (K, 1)
            np.testing.assert_array_equal(g[:, 0], w, err_msg=attr)
    hit = (want.label == 3).astype(np.int32)
    np.testing.assert_array_equal(got.members_hit, hit)
    np.testing.assert_array_equal(_bits(got.risk), _bits(hit.astype(float)))
    assert got.best_members_hit == (0 if want.best >= 0 else -1)
    assert got.best_risk == 0.0 if want.best >= 0 else math.isnan(got.best_risk)
    _against_reference(got, c, EP.decide(c.base, None, 0.0))


# ---- 2. several members ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EP.MULTI) + ["boundary"])
def test_case_against_reference(picker, name):
    c = _case(name)
    for bound in (0.0, 1.0):
        _against_reference(_run(picker, c, None, bound), c, EP.decide(c.base, None, bound))


def test_wavefront_and_member_block_boundaries(picker):
    """The boundary case: a hit at pose 63 in one member and at pose 64 in another, in the first and the last member of each member
    block, and hits at a segment's time index that no pose has -- by construction, not only by the yardstick."""
    c = EP.boundary()
    got = _run(picker, c, None, 0.0)
    B = EP.BOUNDARY_BLOCK
    fp, fs = np.full((4, c.M), -1, np.int32), np.full((4, c.M), -1, np.int32)
    for k, m, i, kind in EP.boundary_plan():
        (fp if kind == "pose" else fs)[k, m] = i
    np.testing.assert_array_equal(got.first_pose_hit, fp)
    np.testing.assert_array_equal(got.first_segment_hit, fs)
    assert list(got.first_pose_hit[0, [0, B - 1, B, 2 * B - 1]]) == [63, 64, 64, 63]
    np.testing.assert_array_equal(got.members_hit, [4, 3, 0, 0])
    assert got.step[0] == 63 and got.step[1] == 62 and got.best == 2


@pytest.mark.parametrize("name", ("long_path_m5", "ragged_m9"))
def test_agrees_with_lifter_and_ensemble_checker(picker, name):
    """Planes and kinematic words are rp_lift_evaluate's bit for bit; first hits and members_hit of the feasible rows are
    rp_ensemble_check's on those planes."""
    from commonroad_rp_amd import EnsembleChecker, TrajectoryLifter
    c = EP.multi(name)
    got = _run(picker, c, None, math.inf)   # (no bound: the status words stay the kinematic ones)
    with TrajectoryLifter(0) as lf, EnsembleChecker(0) as en:
        lf.set_reference(*L.table_args(c.path))
        lifted = lf.lift(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)
        feasible = np.flatnonzero(lifted.status == 1)
        en.set_static(c.obs)
        en.set_members(c.members, c.dyn_t0)
        sub = en.check(c.p, lifted.x[feasible], lifted.y[feasible], lifted.theta[feasible], lengths=None if c.lengths is None else c.lengths[feasible],
                       poses=bool(c.mode & EP.POSES), swept=bool(c.mode & EP.SWEPT))
    for plane in L.PLANES:
        np.testing.assert_array_equal(_bits(getattr(got, plane)), _bits(getattr(lifted, plane)), err_msg=plane)
    np.testing.assert_array_equal(got.status, lifted.status)
    K = len(lifted.status)
    for attr, bit in (("first_pose_hit", EP.POSES), ("first_segment_hit", EP.SWEPT)):
        if c.mode & bit:
            chain = np.full((K, c.M), -1, np.int32)
            chain[feasible] = getattr(sub, attr)
            np.testing.assert_array_equal(getattr(got, attr), chain, err_msg=attr)
    count = np.zeros(K, np.int32)
    count[feasible] = sub.members_hit
    np.testing.assert_array_equal(got.members_hit, count)
    assert got.n_feasible == lifted.n_feasible and got.n_collision == 0


@pytest.mark.parametrize("name", ("long_path_m5", "factor3_m3"))
def test_bound_sweep(picker, name):
    """max_risk 0, 1, ..., M and +inf on the same inputs: what does not depend on the bound is identical across the sweep, the decision
    is the yardstick's at each bound, and the winner moves."""
    c = EP.multi(name)
    _load(picker, c)
    first, winners = None, []
    for bound in [float(q) for q in range(c.M + 1)] + [math.inf]:
        got = _pick(picker, c, bound)
        r = EP.decide(c.base, None, bound)
        _decision_is(got, r, f"{name} at {bound}")
        if r.best >= 0:
            for row, plane in zip(P.PLANE_ROWS, L.PLANES):
                np.testing.assert_array_equal(_bits(got.best_states[row]), _bits(getattr(got, plane)[r.best]))
        first = first or got
        _same_bits(first, got, f"{name} at {bound}", names=UNBOUND, scalars=("n_feasible",))
        winners.append(got.best)
    assert len(set(winners)) > 1 and got.n_collision == 0
    np.testing.assert_array_equal(got.status, c.base.lift.status)


def test_bound_on_the_knife_edge(picker):
    """max_risk set to exactly the bits of a trajectory's risk accepts it; the next double below rejects it."""
    c = EP.multi("long_path_m5")
    w = 0.1 * (1 + np.arange(c.M))
    _load(picker, c, w)
    risk = EP.decide(c.base, w, 0.0).risk
    edges = sorted(set(float(q) for q in risk[(c.base.lift.status == 1) & (risk > 0.0)]))
    assert len(edges) >= 2
    for edge in edges:
        on = np.flatnonzero(risk == edge)
        at, below = _pick(picker, c, edge), _pick(picker, c, float(np.nextafter(edge, -math.inf)))
        assert (at.label[on] == 1).all() and (below.label[on] == 3).all(), edge
        _decision_is(at, EP.decide(c.base, w, edge), f"at {edge!r}")
        _decision_is(below, EP.decide(c.base, w, float(np.nextafter(edge, -math.inf))), f"below {edge!r}")


@pytest.mark.parametrize("name", ("long_path_m5", "long_path_m65", "ragged_m9"))
def test_weights_are_summed_in_ascending_member_order(picker, name):
    """Dyadic weights (multiples of 1 / 64: every order gives the same sum) and 0.1, 0.2, ... (the order shows): bit-equal risks."""
    c = EP.multi(name)
    m = np.arange(c.M)
    for w in ((1 + 3 * m % 7) / 64.0, 0.1 * (1 + m)):
        bound = float(np.sort(w)[: max(1, c.M // 2)].sum())
        got = _run(picker, c, w, bound)
        r = EP.decide(c.base, w, bound)
        np.testing.assert_array_equal(_bits(got.risk), _bits(r.risk), err_msg=name)
        np.testing.assert_array_equal(got.members_hit, r.members_hit)
        _decision_is(got, r, name)
    # a refused weight leaves members and weights in place
    lib = picker._lib
    for bad in (-0.5, math.nan, math.inf):
        wb = np.ones(c.M)
        wb[c.M - 1] = bad
        mem = np.ascontiguousarray(c.members)
        assert lib.rp_epick_set_members(picker._h, c.M, mem.shape[1], mem.shape[2], c.dyn_t0, _capi.dptr(mem), _capi.dptr(wb)) == EINVAL
    again = _pick(picker, c, bound)
    np.testing.assert_array_equal(_bits(again.risk), _bits(r.risk))


def test_a_member_of_weight_zero_counts_and_adds_no_risk(picker):
    c = EP.multi("long_path_m5")
    w = np.ones(c.M)
    w[0] = 0.0
    got = _run(picker, c, w, 0.0)
    r = EP.decide(c.base, w, 0.0)
    _against_reference(got, c, r)
    np.testing.assert_array_equal(got.members_hit, c.base.members_hit)
    np.testing.assert_array_equal(got.risk, c.base.hit[:, 1:].sum(axis=1).astype(float))
    only0 = np.flatnonzero(c.base.hit[:, 0] & (c.base.members_hit == 1))
    assert (got.label[only0] == 1).all()   # hit in the weightless member alone: risk 0, accepted at bound 0
    everywhere = np.zeros(c.M)
    free = _run(picker, c, everywhere, 0.0)
    np.testing.assert_array_equal(free.status, c.base.lift.status)
    assert (free.risk == 0.0).all() and free.n_collision == 0
    np.testing.assert_array_equal(free.members_hit, c.base.members_hit)


# ---- 3. outputs asked for, repeats, sizes ------------------------------------------------------------------------------------------
def _raw(ep, c, mode=None, max_risk=0.0, K=None, n=None, planes=None, lens=None, theta0=None, flags=0, p=None, cost=None, outs=None, status=None,
         cost_out=None, hit=None, risk=None, fp=None, fs=None, result=None, block=None):
    lib, dp = ep._lib, _capi.dptr
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    planes = [np.ascontiguousarray(q) for q in c.planes] if planes is None else planes
    K, n = (planes[0].shape[0] if K is None else K), (planes[0].shape[1] if n is None else n)
    lens = c.lengths if lens is None else lens
    theta0 = c.theta0 if theta0 is None else theta0
    return lib.rp_epick_select(ep._h, C.byref(p or c.p), C.byref(cost or c.cost), c.mode if mode is None else mode, max_risk, K, n,
                               *[q if q is None else dp(q) for q in planes], ip(lens), dp(theta0), flags, *[dp(q) for q in (outs or [None] * 8)],
                               None if status is None else status.ctypes.data_as(C.POINTER(C.c_uint32)), dp(cost_out), ip(hit), dp(risk), ip(fp), ip(fs),
                               None if result is None else C.byref(result), dp(block))


def _result_fields(res):
    return (res.best, _bits(np.float64(res.best_cost)).item(), res.n_feasible, res.n_collision, res.n_collision_before_best, tuple(res.reason_counts),
            res.best_members_hit, _bits(np.float64(res.best_risk)).item())


@pytest.mark.parametrize("name", ("ragged_m9", "long_path_m5"))
def test_which_outputs_are_asked_for_changes_no_other_output(picker, name):
    """The call with every output against the call with NULL planes and against the calls with each single output alone: bit for bit."""
    from commonroad_rp_amd.ensemble_pick import RpEpickResult
    c = EP.multi(name)
    K, n = c.planes[0].shape
    bound = 1.0
    full = _run(picker, c, None, bound)
    _against_reference(full, c, EP.decide(c.base, None, bound))
    without = _pick(picker, c, bound, want_planes=False)
    assert all(getattr(without, plane) is None for plane in L.PLANES)
    _same_bits(full, without, "NULL planes")
    nothing = _pick(picker, c, bound, want_planes=False, want_hits=False)
    assert nothing.first_pose_hit is None and nothing.first_segment_hit is None
    _same_bits(full, nothing, "NULL planes and hits")
    for q, plane in enumerate(L.PLANES):
        out = np.empty((K, n))
        assert _raw(picker, c, max_risk=bound, outs=[out if j == q else None for j in range(8)]) == 0
        np.testing.assert_array_equal(_bits(out), _bits(getattr(full, plane)), err_msg=plane)
    status, cost, hit, risk = np.empty(K, np.uint32), np.empty(K), np.empty(K, np.int32), np.empty(K)
    fp, fs, block = np.empty((K, c.M), np.int32), np.empty((K, c.M), np.int32), np.empty((14, n))
    assert _raw(picker, c, max_risk=bound, status=status) == 0 and _raw(picker, c, max_risk=bound, cost_out=cost) == 0
    assert _raw(picker, c, max_risk=bound, hit=hit) == 0 and _raw(picker, c, max_risk=bound, risk=risk) == 0
    assert _raw(picker, c, max_risk=bound, fp=fp) == 0 and _raw(picker, c, max_risk=bound, fs=fs) == 0
    for got, want in ((status, full.status), (cost, full.cost), (hit, full.members_hit), (risk, full.risk), (fp, full.first_pose_hit),
                      (fs, full.first_segment_hit)):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    res = RpEpickResult()
    assert _raw(picker, c, max_risk=bound, result=res) == 0
    assert _result_fields(res) == (full.best, _bits(np.float64(full.best_cost)).item(), full.n_feasible, full.n_collision, full.n_collision_before_best,
                                   tuple(full.reason_counts), full.best_members_hit, _bits(np.float64(full.best_risk)).item())
    assert _raw(picker, c, max_risk=bound, block=block) == 0
    np.testing.assert_array_equal(_bits(block), _bits(full.best_states))
    assert _raw(picker, c, max_risk=bound) == 0   # nothing at all


def test_repeats_are_bit_identical_and_sizes_do_not_leak(picker):
    from commonroad_rp_amd import EnsemblePicker
    five, one, big, small = EP.multi("long_path_m5"), EP.single("long_path"), EP.single("many"), EP.single("n65")
    first = _run(picker, five, None, 1.0)
    _same_bits(first, _pick(picker, five, 1.0), "repeat")
    after_five = _run(picker, one, None, 0.0)          # M = 5 -> M = 1
    first_big = _run(picker, big, None, 0.0)
    _same_bits(first_big, _pick(picker, big, 0.0), "repeat, K = 1100")
    after_big = _run(picker, small, None, 0.0)         # large K -> small K
    with EnsemblePicker(0) as fresh:
        _same_bits(after_five, _run(fresh, one, None, 0.0), "M = 1 after M = 5")
        _same_bits(after_big, _run(fresh, small, None, 0.0), "small after big")
        _same_bits(first, _run(fresh, five, None, 1.0), "fresh object")
    _against_reference(after_five, one, EP.decide(one.base, None, 0.0))


def test_an_object_never_given_members_has_one_empty_member():
    from commonroad_rp_amd import EnsemblePicker
    c, free = EP.single("all_collide"), EP.single("mode0")   # the same trajectories; without tables every test comes back empty
    with EnsemblePicker(0) as fresh:
        assert fresh.n_members == 1
        fresh.set_reference(*L.table_args(c.path))
        got = fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True, want_hits=True)
        assert got.first_pose_hit.shape == (len(got.status), 1)
        assert (got.first_pose_hit == -1).all() and (got.first_segment_hit == -1).all() and got.n_collision == 0
        assert (got.members_hit == 0).all() and (got.risk == 0.0).all()
        np.testing.assert_array_equal(got.status, free.base.lift.status)
        want_best = EP.decide(free.base, None, 0.0).best
        assert got.best == want_best >= 0 and got.best_members_hit == 0 and got.best_risk == 0.0
        fresh.set_members(EP._empty_members(1), 0)
        _same_bits(got, fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True, want_hits=True), "one empty member")
        fresh.set_static(c.obs)          # the static shapes alone: one member, every feasible trajectory hits
        hit = fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True)
        assert hit.best == -1 and hit.best_members_hit == -1 and math.isnan(hit.best_risk)
        feas = c.base.lift.status == 1
        assert (hit.members_hit[feas] == 1).all() and (hit.risk[feas] == 1.0).all() and (hit.members_hit[~feas] == 0).all()
        fresh.set_static(None)
        assert fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True).best == want_best


def test_device_memory_variants_agree_with_the_lds_variants(picker):
    """long_path_m5 on EP_LF_LDS_ROWS segments (the same inputs, the path one segment shorter behind their reach) and many_static with
    three members and one shape less (the last circle, which nothing touches) run the LDS variants: the verdicts are those of the
    variants that read device memory."""
    c = EP.multi("long_path_m5")
    a = _run(picker, c, None, 1.0)
    picker.set_reference(*L.table_args(L.long_path(EP.LF_LDS_ROWS)))
    b = _pick(picker, c, 1.0)
    for name in ("status", "first_pose_hit", "first_segment_hit", "members_hit", "risk"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    assert a.best == b.best
    for name in L.PLANES:
        assert np.abs(getattr(a, name) - getattr(b, name)).max() <= (L.TOL if name in TIGHT else L.STATE_ATOL), name
    src = P.case("many_static")
    one = EP.single("many_static")
    picker.set_reference(*L.table_args(src.path))
    picker.set_static(src.obs)
    picker.set_members(EP._empty_members(3), 0)
    a = _pick(picker, one, 2.0)
    r1 = EP.decide(one.base, None, 0.0)
    np.testing.assert_array_equal(a.members_hit, 3 * r1.members_hit)   # a static hit counts in every member
    np.testing.assert_array_equal(a.first_pose_hit, np.repeat(r1.first_pose_hit, 3, axis=1))
    np.testing.assert_array_equal(a.first_segment_hit, np.repeat(r1.first_segment_hit, 3, axis=1))
    np.testing.assert_array_equal(a.status, r1.status)
    assert a.best == r1.best and 1 <= a.n_collision < a.n_feasible
    fewer = ObstacleTables(static_obb=src.obs.static_obb, static_tri=src.obs.static_tri, static_circ=src.obs.static_circ[:-1])
    assert len(fewer.static_obb) + len(fewer.static_tri) + len(fewer.static_circ) == EP.CK_LDS_ROWS
    alone = ObstacleTables(static_circ=src.obs.static_circ[-1:])
    assert (P.first_hits(src.p, src.path, alone, src.ref.lift, src.mode)[0] == -1).all()
    picker.set_static(fewer)
    _same_bits(a, _pick(picker, one, 2.0), "many_static")


# ---- 4. edge results, arguments and states -------------------------------------------------------------------------------------------
def test_no_winner_and_no_test(picker):
    from commonroad_rp_amd.ensemble_pick import RpEpickResult
    for name in ("all_collide", "all_infeasible"):
        c = EP.single(name)
        _load(picker, c)
        K, n = c.planes[0].shape
        block, res = np.zeros((14, n)), RpEpickResult()
        assert _raw(picker, c, result=res, block=block) == 0
        assert np.isnan(block).all() and res.best == -1 and np.isnan(res.best_cost) and res.best_members_hit == -1 and np.isnan(res.best_risk)
        assert res.n_collision_before_best == res.n_collision == res.n_feasible == int((c.base.lift.status == 1).sum())
    c = EP.multi("long_path_m5")          # mode 0: no test, every count 0 and every risk 0.0, whatever the members hold
    _load(picker, c)
    got = picker.pick(c.p, c.cost, *c.planes, poses=False, swept=False, want_hits=True)
    assert got.first_pose_hit is None and got.first_segment_hit is None
    assert (got.members_hit == 0).all() and (_bits(got.risk) == 0).all() and got.n_collision == 0 and got.n_collision_before_best == 0
    np.testing.assert_array_equal(got.status, c.base.lift.status)
    feas = c.base.lift.status == 1
    assert got.best == int(np.flatnonzero(feas)[np.argmin(c.base.cost[feas])]) and got.best_members_hit == 0 and got.best_risk == 0.0


def test_argument_errors_and_empty_calls(picker):
    from commonroad_rp_amd import EnsemblePicker
    from commonroad_rp_amd.ensemble_pick import RpEpickResult
    c = EP.multi("factor3_m3")
    t = c.path
    lib = picker._lib
    K, n = c.planes[0].shape
    mem = np.ascontiguousarray(c.members)
    with EnsemblePicker(0) as bare:   # no reference yet: RP_ESTATE, before K == 0 returns; tables alone do not change that
        assert _raw(bare, c, K=0) == ESTATE
        bare.set_static(c.obs)
        bare.set_members(c.members, c.dyn_t0)
        assert _raw(bare, c) == ESTATE
        with pytest.raises(_capi.RpError, match="no reference"):
            bare.pick(c.p, c.cost, *c.planes)
    _load(picker, c)
    res, block = RpEpickResult(), np.zeros((14, n))
    res.best, res.n_feasible, res.n_collision, res.n_collision_before_best, res.best_members_hit, res.best_risk = 7, 7, 7, 7, 7, 7.0
    assert _raw(picker, c, K=0, result=res, block=block) == 0
    assert (res.best, res.n_feasible, res.n_collision, res.n_collision_before_best, res.best_members_hit) == (-1, 0, 0, 0, -1)
    assert np.isnan(res.best_cost) and np.isnan(res.best_risk) and not any(res.reason_counts) and np.isnan(block).all()
    # the bound
    for bad in (math.nan, -1.0, -math.inf, -1e-300):
        assert _raw(picker, c, max_risk=bad) == EINVAL and b"max_risk" in lib.rp_epick_last_error(picker._h)
    assert _raw(picker, c, max_risk=math.inf) == 0 and _raw(picker, c, max_risk=0.0) == 0
    # what rp_pick_select refuses
    assert _raw(picker, c, K=-1) == EINVAL and _raw(picker, c, n=0) == EINVAL and _raw(picker, c, flags=1) == EINVAL
    assert _raw(picker, c, K=(1 << 24) + 1) == EINVAL and _raw(picker, c, K=1 << 13, n=(1 << 11) + 1) == EINVAL
    for hole in range(6):
        planes = [np.ascontiguousarray(q) for q in c.planes]
        planes[hole] = None
        assert _raw(picker, c, planes=planes, K=K, n=n) == EINVAL
    for bad in (0, n + 1):
        assert _raw(picker, c, lens=np.array([n] * (K - 1) + [bad], np.int32)) == EINVAL
    p = _capi.RpParams.from_buffer_copy(c.p)
    p.dt = 0.0
    assert _raw(picker, c, p=p) == EINVAL
    fp, fs = np.empty((K, c.M), np.int32), np.empty((K, c.M), np.int32)
    assert _raw(picker, c, mode=4) == EINVAL and _raw(picker, c, mode=EP.POSES | 8) == EINVAL
    assert _raw(picker, c, mode=EP.SWEPT, fp=fp) == EINVAL and _raw(picker, c, mode=EP.POSES, fs=fs) == EINVAL
    assert _raw(picker, c, mode=0, fp=fp) == EINVAL and _raw(picker, c, mode=0, fs=fs) == EINVAL
    assert _raw(picker, c, mode=EP.SWEPT, fs=fs) == 0 and _raw(picker, c, mode=EP.POSES, fp=fp) == 0
    for kind in (2, 3, -1):
        k = _capi.RpCost.from_buffer_copy(c.cost)
        k.kind = kind
        assert _raw(picker, c, cost=k) == EINVAL
    for field in ("desired_speed", "desired_d", "desired_s"):
        k = _capi.RpCost.from_buffer_copy(c.cost)
        setattr(k, field, float("inf"))
        assert _raw(picker, c, cost=k) == EINVAL
    nulls = [None] * 8
    assert lib.rp_epick_select(picker._h, None, C.byref(c.cost), 0, 0.0, 0, 1, *nulls, 0, *([None] * 16)) == EINVAL
    assert lib.rp_epick_select(picker._h, C.byref(c.p), None, 0, 0.0, 0, 1, *nulls, 0, *([None] * 16)) == EINVAL
    # K * n_members beyond the verdict limit (refused before a plane is read: K * n_poses is within its own limit)
    assert c.M == 3 and _raw(picker, c, K=(1 << 24) // 3 + 1, n=1) == EINVAL and b"VERDICTS" in lib.rp_epick_last_error(picker._h)
    # the three struct sizes
    p = _capi.RpParams.from_buffer_copy(c.p)
    p.struct_size += 8
    assert _raw(picker, c, p=p) == EABI and b"rp_params" in lib.rp_epick_last_error(picker._h)
    k = _capi.RpCost.from_buffer_copy(c.cost)
    k.struct_size += 8
    assert _raw(picker, c, cost=k) == EABI and b"rp_cost" in lib.rp_epick_last_error(picker._h)
    res = RpEpickResult()
    res.struct_size -= 8
    assert _raw(picker, c, result=res) == EABI and b"rp_epick_result" in lib.rp_epick_last_error(picker._h)
    # refused tables leave the earlier ones in place: the reference's, the static shapes', the members'
    pos = t.pos.copy()
    pos[3] = pos[2]
    for a in ((t.ref[:1], t.pos[:1], t.theta[:1], t.curv[:1], t.curv_d[:1], 20.0), (t.ref, pos, t.theta, t.curv, t.curv_d, 20.0),
              (t.ref, t.pos, t.theta, t.curv, t.curv_d, 0.0)):
        with pytest.raises(_capi.RpError, match="-> -1"):
            picker.set_reference(*a)
    circ = np.ones((1, 3))
    assert lib.rp_epick_set_static(picker._h, 0, None, 0, None, -1, _capi.dptr(circ)) == EINVAL
    assert lib.rp_epick_set_static(picker._h, 0, None, 0, None, 1, None) == EINVAL
    assert lib.rp_epick_set_static(picker._h, 0, None, 0, None, (2 ** 31 - 1) // 10 + 1, _capi.dptr(circ)) == EINVAL   # (refused unread)
    assert b"too many" in lib.rp_epick_last_error(picker._h)
    dp = _capi.dptr(mem)
    assert lib.rp_epick_set_members(picker._h, 0, mem.shape[1], mem.shape[2], 0, dp, None) == EINVAL
    assert lib.rp_epick_set_members(picker._h, 4097, 0, 0, 0, None, None) == EINVAL
    assert lib.rp_epick_set_members(picker._h, 1, -1, 1, 0, dp, None) == EINVAL and lib.rp_epick_set_members(picker._h, 1, 1, -1, 0, dp, None) == EINVAL
    assert lib.rp_epick_set_members(picker._h, 3, 1 << 11, 1 << 10, 0, dp, None) == EINVAL      # 3 * 2^21 rows: beyond the limit (refused unread)
    assert lib.rp_epick_set_members(picker._h, 1, 2, 3, 0, None, None) == EINVAL                # null table with rows
    got = _pick(picker, c, 1.0)
    _against_reference(got, c, EP.decide(c.base, None, 1.0))
