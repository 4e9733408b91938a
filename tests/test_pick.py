"""The pick (include/rp_pick.h, commonroad_rp_amd.pick) on the device against the yardstick of tests/_pick.py: the lift's reference
for planes and kinematic status, the scorer's cost function, the oracle's collision tests on the reference's poses, selection and
counts in plain Python.  What these tests rest on -- the yardstick gives the reference planner's own decision on a draw fixture fed
whole, no first hit of a case moves when the vehicle grows or shrinks by 2e-6 m, no rival's cost lies within 1e-9 (relative) of a
winner's, no kinematic verdict within 1e-6 of a bound, and every case holds what its name says -- is checked on the CPU in
tests/test_pick_abi.py.

Shapes: the smallest at which these kernels can go wrong -- one wavefront walks a trajectory 64 poses at a time, (trajectory, chunk)
wavefronts test 64 poses and the segments that start at them, a workgroup is four wavefronts, segment rows and static shapes are
staged in LDS up to a capacity each and read from device memory beyond it, and one workgroup of 1024 threads reduces the verdicts.

  pin 120 x 21                        the reference planner's decision on arc_hv_l1_draw (1 rectangle, 1 triangle, 1 circle, 2 dynamic)
  n63, n64, n65, n129 2 x n           chunk boundaries: the first hit is the last pose of 63, pose 63, pose 64 with segment 63 (the swept
                                      pair that crosses a chunk), pose 128 with segment 127
  ragged 37 x 65, len 1 .. 65         poses beyond len, a partial last workgroup, a length-1 trajectory has no segment
  many 1100 x 21                      more than one pass of the final workgroup: the winner beyond k = 1024, more than 64 colliding
                                      trajectories cheaper than it and others costlier
  factor3 8 x 30                      a dynamic table that starts after the first pose and ends before the last segment: time_step0 + i *
                                      factor for poses, time_step0 + i for segments, indices on both sides of the table
  standstill 4 x 80                   a standstill over poses 60 .. 70, theta0 given: the kept orientation decides a hit
  low_vel 8 x 40                      low_vel_mode = 1
  long_path 16 x 31                   PK_LF_LDS_ROWS + 1 segments: the lift kernel's device-memory variant
  many_static 6 x 30                  PK_CK_LDS_ROWS + 1 static shapes: the collision kernel's device-memory variant
  all_infeasible, all_collide         no winner: best = -1, every collision counts as in front of it, the block is NaN
  no_obstacles, mode0                 tables never given / no test asked for: best is the cost minimum
  duplicates 8 x 21                   the same trajectory at two indices: free, it wins at the lower one; colliding and cheaper, it
                                      counts twice
"""
import ctypes as C

import numpy as np
import pytest

from commonroad_rp_amd import _capi
from commonroad_rp_amd.collision import ObstacleTables

import _lift as L
import _pick as P
import _score as S

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, EABI = -1, -3, -7
TIGHT = ("x", "y", "theta", "theta_cl")   # lengths and angles: 1e-9
SCALARS = ("best", "best_cost", "n_feasible", "n_collision", "n_collision_before_best")
PER_TRAJECTORY = ("status", "cost", "first_pose_hit", "first_segment_hit")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b, what=""):
    """Every output two results both hold equal bit for bit (NaN included)."""
    for name in PER_TRAJECTORY + ("reason_counts", "best_states") + L.PLANES:
        x, y = getattr(a, name), getattr(b, name)
        if name == "best_states":
            assert (x is None) == (y is None), what
        if x is None or y is None:   # (planes and hit arrays a call did not ask for)
            continue
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{what}: {name}")
    for name in SCALARS:
        x, y = getattr(a, name), getattr(b, name)
        assert x == y or (x != x and y != y), (what, name, x, y)


@pytest.fixture(scope="module")
def picker():
    from commonroad_rp_amd import TrajectoryPicker
    with TrajectoryPicker(0) as pk:
        yield pk


def _load(pk, c):
    pk.set_reference(*L.table_args(c.path))
    pk.set_obstacles(c.obs)


def _run(pk, c, want_planes=True, want_hits=True):
    _load(pk, c)
    return pk.pick(c.p, c.cost, *c.planes, lengths=c.lengths, theta0=c.theta0, poses=bool(c.mode & P.POSES), swept=bool(c.mode & P.SWEPT),
                   want_planes=want_planes, want_hits=want_hits)


def _against_reference(got, c):
    """The NaN pattern equal and the eight planes to the lift's tolerances; status, both hit arrays and every scalar EQUAL to the
    yardstick's; the cost within COST_RTOL of the cost function applied to the device's own planes of the same call; the winner's block
    bit-equal to the planes and the inputs."""
    r, o, what = c.ref, c.ref.lift, c.name
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
    np.testing.assert_array_equal(got.status, r.status, err_msg=what)
    np.testing.assert_array_equal(got.label, r.status & 3)
    np.testing.assert_array_equal(got.reason, (r.status >> 4) & 7)
    np.testing.assert_array_equal(got.step, (r.status >> 8) & 0xFFF)
    for name, bit in (("first_pose_hit", P.POSES), ("first_segment_hit", P.SWEPT)):
        if c.mode & bit:
            assert getattr(got, name).dtype == np.int32
            np.testing.assert_array_equal(getattr(got, name), getattr(r, name), err_msg=f"{what}: {name}")
        else:
            assert getattr(got, name) is None
    assert (got.best, got.n_feasible, got.n_collision, got.n_collision_before_best) == (r.best, r.n_feasible, r.n_collision, r.n_collision_before_best), what
    np.testing.assert_array_equal(got.reason_counts, r.reason_counts, err_msg=what)
    # the cost: the cost function on the device's own planes
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
        assert got.best_states is None and np.isnan(got.best_cost)
        return
    assert _bits(np.float64(got.best_cost)) == _bits(got.cost[got.best])
    m = int(o.lengths[r.best])
    block = got.best_states
    assert block.shape == (14, n)
    for row, name in zip(P.PLANE_ROWS, L.PLANES):
        np.testing.assert_array_equal(_bits(block[row]), _bits(getattr(got, name)[r.best]), err_msg=f"{what}: row {row} of the winner's block")
    for row, q in zip(P.INPUT_ROWS, c.planes):
        np.testing.assert_array_equal(_bits(block[row, :m]), _bits(q[r.best, :m]), err_msg=f"{what}: row {row} of the winner's block")
        assert np.isnan(block[row, m:]).all()


# ---- 1. the pin and the shapes -------------------------------------------------------------------------------------------------
def test_pin_is_the_planners_decision(picker):
    c = P.pin()
    got = _run(picker, c)
    _against_reference(got, c)
    e = c.extras
    assert int(c.fixture.index[got.best]) == e.winner and abs(got.best_cost - e.winner_cost) <= S.COST_RTOL * e.winner_cost
    assert got.n_collision_before_best == e.n_infeasible_collision and len(got.status) - got.n_feasible == e.n_infeasible_kinematics
    np.testing.assert_array_equal(got.reason, np.where(got.label == 3, 0, c.fixture.reason))


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_against_reference(picker, name):
    c = P.case(name)
    _against_reference(_run(picker, c), c)


def test_device_memory_variants_agree_with_the_lds_variants(picker):
    """long_path on LF_LDS_ROWS segments (the same inputs, the path one segment shorter behind their reach) and many_static with one
    shape less (the last circle, which nothing touches in either) run the LDS variants: the verdicts are those of the variants that
    read device memory."""
    c = P.case("long_path")
    a = _run(picker, c)
    picker.set_reference(*L.table_args(L.long_path(P.LF_LDS_ROWS)))
    b = picker.pick(c.p, c.cost, *c.planes, poses=True, swept=True, want_planes=True, want_hits=True)
    for name in ("status", "first_pose_hit", "first_segment_hit"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    assert a.best == b.best
    for name in L.PLANES:
        assert np.abs(getattr(a, name) - getattr(b, name)).max() <= (L.TOL if name in TIGHT else L.STATE_ATOL), name
    c = P.case("many_static")
    a = _run(picker, c)
    fewer = ObstacleTables(static_obb=c.obs.static_obb, static_tri=c.obs.static_tri, static_circ=c.obs.static_circ[:-1])
    assert len(fewer.static_obb) + len(fewer.static_tri) + len(fewer.static_circ) == P.CK_LDS_ROWS
    alone = ObstacleTables(static_circ=c.obs.static_circ[-1:])
    assert (P.first_hits(c.p, c.path, alone, c.ref.lift, c.mode)[0] == -1).all()
    picker.set_obstacles(fewer)
    _same_bits(a, picker.pick(c.p, c.cost, *c.planes, poses=True, swept=True, want_planes=True, want_hits=True), "many_static")


# ---- 2. outputs asked for, repeats -------------------------------------------------------------------------------------------------
def _raw(pk, c, mode=None, K=None, n=None, planes=None, lens=None, theta0=None, flags=0, p=None, cost=None, outs=None, status=None, cost_out=None,
         fp=None, fs=None, result=None, block=None):
    lib, dp = pk._lib, _capi.dptr
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    planes = [np.ascontiguousarray(q) for q in c.planes] if planes is None else planes
    K, n = (planes[0].shape[0] if K is None else K), (planes[0].shape[1] if n is None else n)
    lens = c.lengths if lens is None else lens
    theta0 = c.theta0 if theta0 is None else theta0
    return lib.rp_pick_select(pk._h, C.byref(p or c.p), C.byref(cost or c.cost), c.mode if mode is None else mode, K, n,
                              *[q if q is None else dp(q) for q in planes], ip(lens), dp(theta0), flags, *[dp(q) for q in (outs or [None] * 8)],
                              None if status is None else status.ctypes.data_as(C.POINTER(C.c_uint32)), dp(cost_out), ip(fp), ip(fs),
                              None if result is None else C.byref(result), dp(block))


def _result_fields(res):
    return (res.best, _bits(np.float64(res.best_cost)).item(), res.n_feasible, res.n_collision, res.n_collision_before_best, tuple(res.reason_counts))


@pytest.mark.parametrize("name", ("ragged", "n129"))
def test_which_outputs_are_asked_for_changes_no_other_output(picker, name):
    """The call with every output against the call with NULL planes and against the calls with each single output alone: bit for bit."""
    from commonroad_rp_amd.pick import RpPickResult
    c = P.case(name)
    K, n = c.planes[0].shape
    full = _run(picker, c)
    _against_reference(full, c)
    without = _run(picker, c, want_planes=False)
    assert all(getattr(without, name) is None for name in L.PLANES)
    _same_bits(full, without, "NULL planes")
    nothing = _run(picker, c, want_planes=False, want_hits=False)
    assert nothing.first_pose_hit is None and nothing.first_segment_hit is None
    _same_bits(full, nothing, "NULL planes and hits")
    for q, plane in enumerate(L.PLANES):
        out = np.empty((K, n))
        assert _raw(picker, c, outs=[out if j == q else None for j in range(8)]) == 0
        np.testing.assert_array_equal(_bits(out), _bits(getattr(full, plane)), err_msg=plane)
    status, cost, fp, fs, block = np.empty(K, np.uint32), np.empty(K), np.empty(K, np.int32), np.empty(K, np.int32), np.empty((14, n))
    assert _raw(picker, c, status=status) == 0 and _raw(picker, c, cost_out=cost) == 0 and _raw(picker, c, fp=fp) == 0 and _raw(picker, c, fs=fs) == 0
    for got, want in ((status, full.status), (cost, full.cost), (fp, full.first_pose_hit), (fs, full.first_segment_hit)):
        np.testing.assert_array_equal(_bits(got), _bits(want))
    res = RpPickResult()
    assert _raw(picker, c, result=res) == 0
    assert _result_fields(res) == (full.best, _bits(np.float64(full.best_cost)).item(), full.n_feasible, full.n_collision, full.n_collision_before_best,
                                   tuple(full.reason_counts))
    assert _raw(picker, c, block=block) == 0
    np.testing.assert_array_equal(_bits(block), _bits(full.best_states))
    assert _raw(picker, c) == 0   # nothing at all


def test_no_winner_gives_a_nan_block_and_minus_one(picker):
    from commonroad_rp_amd.pick import RpPickResult
    for name in ("all_collide", "all_infeasible"):
        c = P.case(name)
        _load(picker, c)
        K, n = c.planes[0].shape
        block, res = np.zeros((14, n)), RpPickResult()
        assert _raw(picker, c, result=res, block=block) == 0
        assert np.isnan(block).all() and res.best == -1 and np.isnan(res.best_cost)
        assert res.n_collision_before_best == res.n_collision == res.n_feasible == c.ref.n_feasible


def test_repeats_are_bit_identical_and_sizes_do_not_leak(picker):
    from commonroad_rp_amd import TrajectoryPicker
    big, small = P.case("many"), P.case("n65")
    first = _run(picker, big)
    _same_bits(first, _run(picker, big), "repeat")
    after = _run(picker, small)
    with TrajectoryPicker(0) as fresh:
        _same_bits(after, _run(fresh, small), "small after big")
        _same_bits(first, _run(fresh, big), "fresh object")


def test_a_picker_never_given_obstacles_checks_against_empty_tables():
    from commonroad_rp_amd import TrajectoryPicker
    c, free = P.case("all_collide"), P.case("mode0")   # the same trajectories; without tables every test comes back empty
    with TrajectoryPicker(0) as fresh:
        fresh.set_reference(*L.table_args(c.path))
        got = fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True, want_hits=True)
        assert (got.first_pose_hit == -1).all() and (got.first_segment_hit == -1).all() and got.n_collision == 0
        np.testing.assert_array_equal(got.status, free.ref.status)
        assert got.best == free.ref.best >= 0
        fresh.set_obstacles(c.obs)
        assert fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True).best == -1
        fresh.set_obstacles(None)
        assert fresh.pick(c.p, c.cost, *c.planes, poses=True, swept=True).best == free.ref.best


# ---- 3. the chain this call replaces, on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("pin", "many"))
def test_agrees_with_lifter_then_checker(picker, name):
    """TrajectoryLifter.lift_states -> TrajectoryChecker.check gives the labels and the hit arrays of one pick; the poses are bit-equal."""
    from commonroad_rp_amd import TrajectoryChecker, TrajectoryLifter
    c = P.pin() if name == "pin" else P.case(name)
    got = _run(picker, c)
    with TrajectoryLifter(0) as lf, TrajectoryChecker(0) as ck:
        lf.set_reference(*L.table_args(c.path))
        lifted = lf.lift(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)
        states = lf.lift_states(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)
        ck.set_obstacles(c.obs)
        feasible = np.flatnonzero(lifted.status == 1)
        sub = ck.check(c.p, states[feasible, 0], states[feasible, 1], states[feasible, 2], lengths=None if c.lengths is None else c.lengths[feasible],
                       poses=bool(c.mode & P.POSES), swept=bool(c.mode & P.SWEPT))
    for plane in L.PLANES:
        np.testing.assert_array_equal(_bits(getattr(got, plane)), _bits(getattr(lifted, plane)), err_msg=plane)
    label = lifted.status & 3
    K = len(label)
    for attr, bit in (("first_pose_hit", P.POSES), ("first_segment_hit", P.SWEPT)):
        if c.mode & bit:
            chain = np.full(K, -1, np.int32)
            chain[feasible] = getattr(sub, attr)
            np.testing.assert_array_equal(getattr(got, attr), chain, err_msg=attr)
            label = np.where(chain >= 0, 3, label)
    np.testing.assert_array_equal(got.label, label)
    np.testing.assert_array_equal(got.status[label == 2], lifted.status[label == 2])
    assert got.n_collision == sub.n_hit and got.n_feasible == lifted.n_feasible


# ---- 4. arguments and states -------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_calls(picker):
    from commonroad_rp_amd import TrajectoryPicker
    from commonroad_rp_amd.pick import RpPickResult
    c = P.case("n63")
    t = c.path
    lib = picker._lib
    K, n = c.planes[0].shape
    with TrajectoryPicker(0) as bare:   # no reference yet: RP_ESTATE, before K == 0 returns; obstacles alone do not change that
        assert _raw(bare, c, K=0) == ESTATE
        bare.set_obstacles(c.obs)
        assert _raw(bare, c) == ESTATE
        with pytest.raises(_capi.RpError, match="no reference"):
            bare.pick(c.p, c.cost, *c.planes)
    _load(picker, c)
    res, block = RpPickResult(), np.zeros((14, n))
    res.best, res.n_feasible, res.n_collision, res.n_collision_before_best = 7, 7, 7, 7
    assert _raw(picker, c, K=0, result=res, block=block) == 0
    assert (res.best, res.n_feasible, res.n_collision, res.n_collision_before_best) == (-1, 0, 0, 0) and np.isnan(res.best_cost)
    assert not any(res.reason_counts) and np.isnan(block).all()
    # what rp_lift_evaluate refuses
    assert _raw(picker, c, K=-1) == EINVAL and _raw(picker, c, n=0) == EINVAL and _raw(picker, c, flags=1) == EINVAL
    assert _raw(picker, c, K=(1 << 24) + 1) == EINVAL and _raw(picker, c, K=1 << 13, n=(1 << 11) + 1) == EINVAL
    for hole in range(6):
        planes = [np.ascontiguousarray(q) for q in c.planes]
        planes[hole] = None
        assert _raw(picker, c, planes=planes, K=K, n=n) == EINVAL
    for bad in (0, n + 1):
        assert _raw(picker, c, lens=np.array([n, bad], np.int32)) == EINVAL
    p = _capi.RpParams.from_buffer_copy(c.p)
    p.dt = 0.0
    assert _raw(picker, c, p=p) == EINVAL
    # what rp_checker_check refuses, and the mode bits
    fp, fs = np.empty(K, np.int32), np.empty(K, np.int32)
    assert _raw(picker, c, mode=4) == EINVAL and _raw(picker, c, mode=P.POSES | 8) == EINVAL
    assert _raw(picker, c, mode=P.SWEPT, fp=fp) == EINVAL and _raw(picker, c, mode=P.POSES, fs=fs) == EINVAL
    assert _raw(picker, c, mode=0, fp=fp) == EINVAL and _raw(picker, c, mode=0, fs=fs) == EINVAL
    assert _raw(picker, c, mode=P.SWEPT, fs=fs) == 0 and _raw(picker, c, mode=P.POSES, fp=fp) == 0
    # the cost
    for kind in (2, 3, -1):
        k = _capi.RpCost.from_buffer_copy(c.cost)
        k.kind = kind
        assert _raw(picker, c, cost=k) == EINVAL
    for field in ("desired_speed", "desired_d", "desired_s"):
        k = _capi.RpCost.from_buffer_copy(c.cost)
        setattr(k, field, float("inf"))
        assert _raw(picker, c, cost=k) == EINVAL
    assert lib.rp_pick_select(picker._h, None, C.byref(c.cost), 0, 0, 1, *([None] * 8), 0, *([None] * 14)) == EINVAL
    assert lib.rp_pick_select(picker._h, C.byref(c.p), None, 0, 0, 1, *([None] * 8), 0, *([None] * 14)) == EINVAL
    # the three struct sizes
    p = _capi.RpParams.from_buffer_copy(c.p)
    p.struct_size += 8
    assert _raw(picker, c, p=p) == EABI and b"rp_params" in lib.rp_pick_last_error(picker._h)
    k = _capi.RpCost.from_buffer_copy(c.cost)
    k.struct_size += 8
    assert _raw(picker, c, cost=k) == EABI and b"rp_cost" in lib.rp_pick_last_error(picker._h)
    res = RpPickResult()
    res.struct_size -= 8
    assert _raw(picker, c, result=res) == EABI and b"rp_pick_result" in lib.rp_pick_last_error(picker._h)
    # the fail-safe cost is accepted
    k = _capi.make_cost(kind=1)
    costs, outs = np.empty(K), [np.empty((K, n)) for _ in range(8)]
    assert _raw(picker, c, cost=k, cost_out=costs, outs=outs) == 0
    for q in np.flatnonzero(c.ref.lift.status == 1):
        want = S.cost_of(k, outs[4][q], outs[3][q], c.planes[0][q], c.planes[3][q], outs[7][q])
        assert abs(costs[q] - want) <= S.COST_RTOL * want
    # refused tables leave the earlier ones in place: the reference's five refusals and two of the obstacles'
    pos = t.pos.copy()
    pos[3] = pos[2]
    xy = t.ref.copy()
    xy[5] = xy[4]
    curv = t.curv.copy()
    curv[1] = np.nan
    for a in ((t.ref[:1], t.pos[:1], t.theta[:1], t.curv[:1], t.curv_d[:1], 20.0), (t.ref, pos, t.theta, t.curv, t.curv_d, 20.0),
              (xy, t.pos, t.theta, t.curv, t.curv_d, 20.0), (t.ref, t.pos, t.theta, curv, t.curv_d, 20.0),
              (t.ref, t.pos, t.theta, t.curv, t.curv_d, 0.0), (t.ref, t.pos, t.theta, t.curv, t.curv_d, float("inf"))):
        with pytest.raises(_capi.RpError, match="-> -1"):
            picker.set_reference(*a)
    circ = np.ascontiguousarray(c.obs.static_circ)
    assert lib.rp_pick_set_obstacles(picker._h, 0, None, 0, None, -1, _capi.dptr(circ), 0, 0, 0, None) == EINVAL
    assert lib.rp_pick_set_obstacles(picker._h, 0, None, 0, None, 1, None, 0, 0, 0, None) == EINVAL
    assert lib.rp_pick_set_obstacles(picker._h, 0, None, 0, None, 0, None, 2, 3, 0, None) == EINVAL
    assert lib.rp_pick_set_obstacles(picker._h, 0, None, 0, None, (2 ** 31 - 1) // 10 + 1, _capi.dptr(circ), 0, 0, 0, None) == EINVAL   # (refused unread)
    assert b"too many" in lib.rp_pick_last_error(picker._h)
    got = picker.pick(c.p, c.cost, *c.planes, poses=True, swept=True, want_planes=True, want_hits=True)
    _against_reference(got, c)
