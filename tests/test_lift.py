"""The lift (include/rp_lift.h, commonroad_rp_amd.lift) on the device against the draw fixtures and the NumPy reference of
tests/_lift.py.  What these tests rest on -- the reference reproduces the fixtures' Cartesian rows and reasons, its points are
CoordinateSystem.convert_to_cartesian_coords, no verdict of a case comes within 1e-6 of a threshold and every synthetic case holds
what its name says -- is checked on the CPU in tests/test_lift_abi.py.

Shapes: the smallest at which these kernels can go wrong -- a wavefront walks one trajectory 64 poses at a time and hands theta, kappa
and the orientation a standstill keeps from one chunk to the next, a workgroup is four wavefronts, segment rows are staged in LDS up
to a capacity and read from device memory beyond it, and one workgroup of 1024 threads reduces the verdicts.

  one_pose 3 x 1                      rates at i = 0 only; theta0 per trajectory
  n63, n64, n65, n129 1 x n           chunk boundaries of the 64-pose wavefront
  ragged 37 x 65, len 1 .. 65         poses beyond len, a partial last workgroup
  standstill_head(_theta0) 4 x 20     s_dot = 0 from pose 0: theta = theta0, NULL and given
  standstill_across 2 x 80            a standstill over poses 60 .. 70: the carry crosses a chunk
  standstill_all 1 x 70               never moves
  stop_and_go 3 x 66                  two standstills in one trajectory, the second across the chunk boundary
  low_vel 8 x 40                      low_vel_mode = 1 with poses at s_dot <= 0.001 (no carry)
  off_end, off_start 4 x 30           s leaves the path mid-way, or starts below it: NaN from there, reason 6 unless an earlier step failed
  vertex_hits 1 x n_vertices          s exactly on every vertex, the last included
  beyond_d 4 x 20                     |d| beyond the limit on a trajectory that passes the kinematics, and on one that fails earlier
  nan_input 3 x 10                    a NaN in s, in d, in s_dot
  long_path(_at_cap) 16 x 31          the same inputs on paths of LF_LDS_ROWS + 1 (device-memory table) and LF_LDS_ROWS segments
  many 1100 x 21                      more trajectories than one pass of the final kernel's workgroup; first_feasible is not 0
"""
import ctypes as C

import numpy as np
import pytest

from commonroad_rp_amd import _capi

import _lift as R
import _score as S

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, EABI = -1, -3, -7
TIGHT = ("x", "y", "theta", "theta_cl")   # lengths and angles: 1e-9


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same_bits(a, b):
    """Every output of two results equal bit for bit (NaN included)."""
    for name in ("status", "reason_counts") + R.PLANES:
        np.testing.assert_array_equal(_bits(getattr(a, name)), _bits(getattr(b, name)), err_msg=name)
    assert (a.first_feasible, a.n_feasible) == (b.first_feasible, b.n_feasible)


@pytest.fixture(scope="module")
def lifter():
    from commonroad_rp_amd import TrajectoryLifter
    with TrajectoryLifter(0) as lf:
        yield lf


def _run_case(lf, c):
    lf.set_reference(*R.table_args(c.path))
    return lf.lift(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)


def _run_fixture(lf, name, p=None):
    lf.set_reference(*R.table_args(R.fixture_path(name)))
    q = R.fixture_inputs(name)
    return lf.lift(p or S.fixture(name).p, q["s"], q["s_dot"], q["s_ddot"], q["d"], q["d_dot"], q["d_ddot"], lengths=q["lengths"])


def _against_reference(got, o, what):
    """The NaN pattern equal; the eight planes to 1e-6, x, y, theta and theta_cl to 1e-9; status words and the reductions equal."""
    worst = {}
    for name in R.PLANES:
        g, w = getattr(got, name), getattr(o, name)
        assert g.shape == w.shape and g.dtype == np.float64
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: NaN pattern of {name}")
        fin = ~np.isnan(w)
        worst[name] = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
    print(f"{what}: largest |device - reference| " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= (R.TOL if name in TIGHT else R.STATE_ATOL), (what, name, v)
    np.testing.assert_array_equal(got.status, o.status, err_msg=what)
    assert (got.first_feasible, got.n_feasible) == (o.first_feasible, o.n_feasible), what
    np.testing.assert_array_equal(got.reason_counts, o.reason_counts, err_msg=what)
    np.testing.assert_array_equal(got.label, o.status & 3)
    np.testing.assert_array_equal(got.reason, (o.status >> 4) & 7)
    np.testing.assert_array_equal(got.step, (o.status >> 8) & 0xFFF)


# ---- 1. the pins, through the library ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GPU_FIXTURES)
def test_fixture_rows_and_verdicts(lifter, name):
    f, o = S.fixture(name), R.fixture_reference(name)
    got = _run_fixture(lifter, name)
    _against_reference(got, o, name)
    valid = np.arange(f.n)[None, :] < f.lengths[:, None]   # ... and to the fixture itself
    for pl, row in (("x", 0), ("y", 1), ("theta", 2), ("v", 3), ("a", 4), ("kappa", 5), ("kappa_dot", 6), ("theta_cl", R.RP_THETA_CL)):
        assert np.abs(getattr(got, pl) - f.states[:, row])[valid].max() <= (R.TOL if pl in TIGHT else R.STATE_ATOL), pl
    np.testing.assert_array_equal(got.reason, f.reason)
    np.testing.assert_array_equal(got.label == 1, f.reason == 0)


# ---- 2. the shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_against_reference(lifter, name):
    c = R.case(name)
    _against_reference(_run_case(lifter, c), c.out, name)


def test_long_path_variants_agree(lifter):
    """The same inputs through the LDS table and through the device-memory table: the paths differ behind the inputs' reach alone (one
    more segment at the far end), so the rows agree to rounding of the tables' own construction and the verdicts are equal."""
    a, b = _run_case(lifter, R.case("long_path")), _run_case(lifter, R.case("long_path_at_cap"))
    np.testing.assert_array_equal(a.status, b.status)
    for name in R.PLANES:
        assert np.abs(getattr(a, name) - getattr(b, name)).max() <= (R.TOL if name in TIGHT else R.STATE_ATOL), name


# ---- 3. points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("cfg2_ref_draw", "long_path", "u_limit"))
def test_points_against_reference(lifter, path):
    rng = np.random.default_rng(17)
    t = R.fixture_path(path) if path == "cfg2_ref_draw" else R.long_path(R.LDS_ROWS + 1) if path == "long_path" else R.built_path(S.U_PATH, d_limit=1.5)
    s = np.concatenate((t.pos, [np.nextafter(t.pos[0], -np.inf), np.nextafter(t.pos[-1], np.inf), np.nan, np.inf, t.pos[0], t.pos[-1]],
                        rng.uniform(t.pos[0] - 1.0, t.pos[-1] + 1.0, 300)))
    s = s[:s.size // 2 * 2]
    d = rng.uniform(-1.1 * t.d_limit, 1.1 * t.d_limit, s.size)
    d[:8] = [t.d_limit, -t.d_limit, np.nextafter(t.d_limit, np.inf), np.nan, 0.0, 0.0, -np.inf, 0.0]
    lifter.set_reference(*R.table_args(t))
    x, y, seg, n_out = lifter.points(s, d, want_outside=True)
    wx, wy, wseg = R.points(t, s, d)
    np.testing.assert_array_equal(seg, wseg)
    np.testing.assert_array_equal(np.isnan(x), wseg < 0)
    np.testing.assert_array_equal(np.isnan(y), wseg < 0)
    on = wseg >= 0
    assert n_out == int((~on).sum()) and 10 <= n_out <= s.size - 50
    worst = max(float(np.abs(x[on] - wx[on]).max()), float(np.abs(y[on] - wy[on]).max()))
    print(f"{path}: largest |device - reference| of a position {worst:.1e} m over {int(on.sum())} points, {n_out} off the path")
    assert worst <= R.TOL
    x2, y2, seg2 = lifter.points(s.reshape(2, -1), d.reshape(2, -1))   # the shape of the input comes back
    assert x2.shape == (2, s.size // 2) and np.array_equal(_bits(x2.ravel()), _bits(x)) and np.array_equal(seg2.ravel(), seg)
    e = lifter.points(np.empty(0), np.empty(0), want_outside=True)
    assert e[0].shape == (0,) and e[3] == 0


# ---- 4. masks, NULL outputs, repeats -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", (0, 1, 2, 4, 8, 16))
def test_single_check_masks(lifter, mask):
    name = "cfg1_ref_l1_draw"
    p = _capi.RpParams.from_buffer_copy(S.fixture(name).p)
    p.constraint_mask = mask
    o = R.reference(p, R.fixture_path(name), **R.fixture_inputs(name))
    got = _run_fixture(lifter, name, p)
    _against_reference(got, o, f"mask {mask}")
    if mask:
        assert set(got.reason.tolist()) <= {0, {1: 1, 2: 2, 4: 3, 8: 4, 16: 5}[mask]}
    else:
        assert got.n_feasible == len(got.status) and got.first_feasible == 0


def _raw(lifter, c, outs=None, status=None, first=None, n_feasible=None, counts=None, K=None, n=None, flags=0, p=None, planes=None, lens=None):
    lib, dp = lifter._lib, _capi.dptr
    planes = [np.ascontiguousarray(q) for q in c.planes] if planes is None else planes
    K, n = (planes[0].shape[0] if K is None else K), (planes[0].shape[1] if n is None else n)
    outs = outs or [None] * 8
    return lib.rp_lift_evaluate(lifter._h, C.byref(p or c.p), K, n, *[q if q is None else dp(q) for q in planes],
                                None if lens is None else lens.ctypes.data_as(C.POINTER(C.c_int32)), None, flags, *[dp(q) for q in outs],
                                None if status is None else status.ctypes.data_as(C.POINTER(C.c_uint32)), first, n_feasible,
                                None if counts is None else counts.ctypes.data_as(C.POINTER(C.c_int64)))


def test_null_output_pointers(lifter):
    c = R.case("ragged")
    lifter.set_reference(*R.table_args(c.path))
    planes = [np.ascontiguousarray(q[:, :40]) for q in c.planes]   # (no lengths: all 40 poses)
    o = R.reference(c.p, c.path, *planes)
    nf = C.c_int64(-5)
    assert _raw(lifter, c, planes=planes, n_feasible=C.byref(nf)) == 0 and nf.value == o.n_feasible
    status, nf2, ff, counts = np.zeros(37, np.uint32), C.c_int64(-5), C.c_int64(-5), np.full(8, -1, np.int64)
    assert _raw(lifter, c, planes=planes, status=status) == 0
    np.testing.assert_array_equal(status, o.status)
    kappa = np.empty((37, 40))
    assert _raw(lifter, c, planes=planes, outs=[None] * 5 + [kappa, None, None], first=C.byref(ff), n_feasible=C.byref(nf2), counts=counts) == 0
    assert (ff.value, nf2.value) == (o.first_feasible, o.n_feasible) and np.array_equal(counts, o.reason_counts)
    assert np.abs(kappa - o.kappa).max() <= R.STATE_ATOL


def test_repeats_are_bit_identical_and_sizes_do_not_leak(lifter):
    from commonroad_rp_amd import TrajectoryLifter
    big, small = R.case("many"), R.case("n65")
    first = _run_case(lifter, big)
    _same_bits(first, _run_case(lifter, big))
    after = _run_case(lifter, small)
    with TrajectoryLifter(0) as fresh:
        _same_bits(after, _run_case(fresh, small))
        _same_bits(first, _run_case(fresh, big))


# ---- 5. the chain: lift -> score ---------------------------------------------------------------------------------------------------
def test_round_trip_through_the_scorer(lifter):
    """lift_states of cfg2_ref_draw, handed to TrajectoryScorer.score_states on the same path, comes back with the s and d it was lifted
    from and with theta_cl on the poses whose theta_cl the lift wrapped (a moving pose's atan2 lies within (-pi/2, pi/2); a standstill's
    difference is left unwrapped), to 1e-9; and the scorer's kinematic verdict on the lifted rows is the lift's."""
    from commonroad_rp_amd import TrajectoryScorer
    name = "cfg2_ref_draw"
    f, t, q = S.fixture(name), R.fixture_path(name), R.fixture_inputs(name)
    lifter.set_reference(*R.table_args(t))
    args = (q["s"], q["s_dot"], q["s_ddot"], q["d"], q["d_dot"], q["d_ddot"])
    states = lifter.lift_states(f.p, *args, lengths=q["lengths"])
    got = lifter.lift(f.p, *args, lengths=q["lengths"])
    assert states.shape == (len(f.index), 14, f.n)
    for row, plane in ((0, got.x), (5, got.kappa), (6, got.kappa_dot), (9, got.theta_cl), (7, q["s"]), (13, q["d_ddot"])):
        np.testing.assert_array_equal(_bits(states[:, row]), _bits(np.ascontiguousarray(plane)))
    with TrajectoryScorer(0) as sc:
        sc.set_reference(t.ref, t.pos, t.theta, t.d_limit)
        back = sc.score_states(f.p, f.cost, states, lengths=q["lengths"], want_states=True)
    valid = np.arange(f.n)[None, :] < q["lengths"][:, None]
    assert not np.isnan(back.s[valid]).any()
    moving = valid & (q["s_dot"] > 0.001)
    worst = [float(np.abs(back.s - q["s"])[valid].max()), float(np.abs(back.d - q["d"])[valid].max()),
             float(np.abs(back.theta_cl - got.theta_cl)[moving].max())]
    print(f"round trip: s {worst[0]:.1e} m, d {worst[1]:.1e} m, theta_cl {worst[2]:.1e} rad over {int(valid.sum())} poses ({int(moving.sum())} moving)")
    assert max(worst) <= R.TOL and moving.sum() > 1000
    np.testing.assert_array_equal(back.status, got.status)


# ---- 6. arguments and states -------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_calls(lifter):
    from commonroad_rp_amd import TrajectoryLifter
    c = R.case("one_pose")
    t = c.path
    lib, dp = lifter._lib, _capi.dptr
    with TrajectoryLifter(0) as bare:   # no reference yet: RP_ESTATE, before K == 0 returns
        assert _raw(bare, c, K=0) == ESTATE
        assert lib.rp_lift_points(bare._h, 0, None, None, None, None, None, None) == ESTATE
        with pytest.raises(_capi.RpError, match="no reference"):
            bare.lift(c.p, *c.planes)
    lifter.set_reference(*R.table_args(t))
    ff, nf, counts = C.c_int64(7), C.c_int64(7), np.full(8, 7, np.int64)
    assert _raw(lifter, c, K=0, first=C.byref(ff), n_feasible=C.byref(nf), counts=counts) == 0
    assert (ff.value, nf.value) == (-1, 0) and not counts.any()
    assert _raw(lifter, c, K=-1) == EINVAL and _raw(lifter, c, n=0) == EINVAL and _raw(lifter, c, flags=1) == EINVAL
    assert _raw(lifter, c, K=(1 << 24) + 1) == EINVAL and _raw(lifter, c, K=1 << 13, n=(1 << 11) + 1) == EINVAL
    for hole in range(6):
        planes = [np.ascontiguousarray(q) for q in c.planes]
        planes[hole] = None
        assert _raw(lifter, c, planes=planes, K=3, n=1) == EINVAL
    for bad in (0, 2):
        assert _raw(lifter, c, lens=np.array([1, bad, 1], np.int32)) == EINVAL
    p = _capi.RpParams.from_buffer_copy(c.p)
    p.dt = 0.0
    assert _raw(lifter, c, p=p) == EINVAL
    p = _capi.RpParams.from_buffer_copy(c.p)
    p.struct_size += 8
    assert _raw(lifter, c, p=p) == EABI
    assert b"struct_size" in lib.rp_lift_last_error(lifter._h)
    # set_reference: the five refusals; the table of before stays in place
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
            lifter.set_reference(*a)
    _against_reference(lifter.lift(c.p, *c.planes, theta0=c.theta0), c.out, "after refused tables")
