"""The clearance query (include/rp_clearance.h, commonroad_rp_amd.clearance) on the device against the NumPy reference of
tests/_clearance.py, and its zeros against the batch collision checker on the same tables.  What these tests rest on -- reference
zero <=> oracle hit on every pose, no reference distance next to 0, to the cutoff or to the margin -- is checked on the CPU in
tests/test_clearance_abi.py.

Shapes: the checker's, the smallest at which this kernel can go wrong -- a wavefront is 64 consecutive poses of one trajectory, a
workgroup four wavefronts, static shapes are staged in LDS up to a capacity and read from device memory beyond it."""
import ctypes as C
import math

import numpy as np
import pytest

from commonroad_rp_amd.collision import ObstacleTables

import _clearance as R

pytestmark = pytest.mark.gpu
INF = math.inf


class _Run:
    pass


@pytest.fixture(scope="module")
def runs():
    """Every case once through the device: the query without a cutoff (every output) and the checker's per-pose verdicts."""
    from commonroad_rp_amd import ClearanceQuery, TrajectoryChecker
    out = []
    with ClearanceQuery(0) as q, TrajectoryChecker(0) as ck:
        for c in R.cases():
            r = _Run()
            q.set_obstacles(c.obs)
            ck.set_obstacles(c.obs)
            r.full = q.query(c.p, c.x, c.y, c.th, lengths=c.lengths, want_pose_clearance=True)
            r.check = ck.check(c.p, c.x, c.y, c.th, lengths=c.lengths, poses=True, swept=False, want_pose_hits=True)
            out.append(r)
    return out


def _reduce(pc):
    """(min_clearance, min_pose) of per-pose clearances [K, n]: the minimum and the smallest pose that attains it, -1 for +inf."""
    m = pc.min(axis=1)
    return m, np.where(np.isinf(m), -1, pc.argmin(axis=1)).astype(np.int32)


def _scalars(min_clear, margin):
    clear = np.flatnonzero(min_clear > margin)
    return (int(clear[0]) if len(clear) else -1, int((min_clear <= margin).sum()), int(np.argmax(min_clear)) if len(min_clear) else -1)


def test_pose_clearance_matches_reference(runs):
    worst = 0.0
    for c, r in zip(R.cases(), runs):
        pc = r.full.pose_clearance
        assert pc.shape == c.clear.shape
        np.testing.assert_array_equal(np.isinf(pc), np.isinf(c.clear))
        assert not np.isnan(pc).any() and (pc >= 0.0).all()
        fin = np.isfinite(pc)
        diff = np.abs(pc[fin] - c.clear[fin])
        worst = max(worst, float(diff.max()) if diff.size else 0.0)
    print(f"largest |device - reference| over all cases: {worst:.3e} m")
    assert worst <= R.TOL


def test_zero_is_the_checkers_hit(runs):
    """pose_clearance == 0.0 exactly where TrajectoryChecker reports a hit on the same tables, > 0 elsewhere (+inf included)."""
    hits = 0
    for c, r in zip(R.cases(), runs):
        np.testing.assert_array_equal(r.full.pose_clearance == 0.0, r.check.pose_hits)
        assert (r.full.pose_clearance[~r.check.pose_hits] > 0.0).all()
        hits += int(r.check.pose_hits.sum())
    assert hits >= 100


def test_trajectory_reductions(runs):
    """min_clearance, min_pose and nearest are the reductions of the device's own pose_clearance; the obstacle named has a reference
    distance within the tolerance of the reference minimum at that pose."""
    for c, r in zip(R.cases(), runs):
        m, at = _reduce(r.full.pose_clearance)
        np.testing.assert_array_equal(r.full.min_clearance, m)
        np.testing.assert_array_equal(r.full.min_pose, at)
        assert r.full.min_clearance.dtype == np.float64 and r.full.min_pose.dtype == np.int32 and r.full.nearest.dtype == np.int32
        for k in range(len(m)):
            j = int(r.full.nearest[k])
            if at[k] < 0:
                assert j == -1
                continue
            row = c.D[k, at[k]]
            assert 0 <= j < len(row) and abs(row[j] - row.min()) <= R.TOL, (k, j)
            if row.min() > 0.0 and (np.sort(row)[1] - row.min() > 2 * R.TOL if len(row) > 1 else True):
                assert j == int(row.argmin())   # a unique nearest obstacle: its id


def test_scalars_and_the_checkers_counts(runs):
    from commonroad_rp_amd import ClearanceQuery
    with ClearanceQuery(0) as q:
        for c, r in zip(R.cases(), runs):
            q.set_obstacles(c.obs)
            assert (r.full.first_clear, r.full.n_below, r.full.best) == _scalars(r.full.min_clearance, 0.0)
            assert (r.full.first_clear, r.full.n_below) == (r.check.first_free, r.check.n_hit)
            s = q.query(c.p, c.x, c.y, c.th, lengths=c.lengths, margin=R.MARGIN)
            assert s.pose_clearance is None
            np.testing.assert_array_equal(s.min_clearance, r.full.min_clearance)
            assert (s.first_clear, s.n_below, s.best) == _scalars(s.min_clearance, R.MARGIN)
            assert s.best == r.full.best
    # the margin tells something the boolean answer does not, somewhere
    assert any(_scalars(r.full.min_clearance, R.MARGIN)[1] > r.full.n_below for r in runs)


def test_cutoff_changes_no_value_at_or_below_it(runs):
    """Every value <= cutoff is bit-equal to the run without a cutoff (pruning changes nothing); every other value is +inf, with nearest
    id -1 where a whole trajectory stays above the cutoff."""
    from commonroad_rp_amd import ClearanceQuery
    kept = dropped = 0
    with ClearanceQuery(0) as q:
        for c, r in zip(R.cases(), runs):
            q.set_obstacles(c.obs)
            s = q.query(c.p, c.x, c.y, c.th, lengths=c.lengths, cutoff=R.CUTOFF, margin=R.MARGIN, want_pose_clearance=True)
            full = r.full.pose_clearance
            near = full <= R.CUTOFF
            np.testing.assert_array_equal(s.pose_clearance[near].view(np.uint64), full[near].view(np.uint64))
            assert np.isinf(s.pose_clearance[~near]).all()
            kept, dropped = kept + int(near.sum()), dropped + int((np.isfinite(full) & ~near).sum())
            m, at = _reduce(s.pose_clearance)
            np.testing.assert_array_equal(s.min_clearance, m)
            np.testing.assert_array_equal(s.min_pose, at)
            below = r.full.min_clearance <= R.CUTOFF
            np.testing.assert_array_equal(s.nearest[below], r.full.nearest[below])
            assert (s.nearest[~below] == -1).all() and (s.min_pose[~below] == -1).all()
            assert (s.first_clear, s.n_below, s.best) == _scalars(s.min_clearance, R.MARGIN)
    assert kept >= 100 and dropped >= 100


def _straight(xs, n_traj=1, dy=100.0):
    """Trajectories along x at the given rear-axle positions, heading 0, dy apart."""
    x = np.tile(np.asarray(xs, float), (n_traj, 1))
    return x, np.tile(dy * np.arange(n_traj)[:, None], (1, x.shape[1])), np.zeros_like(x)


def test_exact_ties():
    from commonroad_rp_amd import ClearanceQuery
    p = R._params(time_step0=0, factor=1, n=6)
    box = [30.0 + R.WB, 4.0, 0.4, 1.0, 0.5]
    disc = [30.0 + R.WB, 0.0, 1.0]
    with ClearanceQuery(0) as q:
        # two identical obstacles, static and dynamic, at a positive distance: the smaller id
        x, y, th = _straight(10.0 * np.arange(6))
        dyn = np.tile(np.array(box)[None, None, :], (2, 6, 1))
        for obs, want in ((ObstacleTables(static_obb=[[500.0, 0.0, 0.0, 1.0, 1.0], box, box]), 1),
                          (ObstacleTables(static_obb=[[500.0, 0.0, 0.0, 1.0, 1.0]], dyn_obb=dyn), 1),
                          (ObstacleTables(static_tri=[[31.0, 5.0, 33.0, 5.0, 32.0, 7.0]] * 2, static_circ=[[500.0, 0.0, 1.0]]), 0)):
            q.set_obstacles(obs)
            r = q.query(p, x, y, th, want_pose_clearance=True)
            assert r.min_pose[0] == 3 and r.nearest[0] == want and 0.0 < r.min_clearance[0] < 5.0
        # a pose inside two obstacles: the smaller id, whatever lies closer to the centre
        for obs, want in ((ObstacleTables(static_obb=[[500.0, 0.0, 0.0, 1.0, 1.0], [31.0, 0.5, 0.3, 3.0, 3.0]], static_circ=[disc]), 1),
                          (ObstacleTables(static_circ=[disc, disc]), 0),
                          (ObstacleTables(static_circ=[[500.0, 0.0, 1.0]], dyn_obb=np.tile(np.array([30.0 + R.WB, 0.0, 0.0, 1.0, 1.0])[None, None, :], (3, 6, 1))), 1)):
            q.set_obstacles(obs)
            r = q.query(p, x, y, th, want_pose_clearance=True)
            assert r.min_clearance[0] == 0.0 and r.min_pose[0] == 3 and r.nearest[0] == want
        # two poses with bit-equal clearance (the same pose twice): the smaller pose -- inside one lane's stride (5 | 69), across lanes
        # of one wavefront (70 | 3) and across wavefronts (100 | 129)
        q.set_obstacles(ObstacleTables(static_circ=[[5.0 + R.WB, 106.0, 1.0]]))   # 4.2 m above trajectory 1 at x = 5
        n = 130
        xs = 1000.0 + 10.0 * np.arange(n)
        for pair in ((5, 69), (70, 3), (100, 129), (0, 64), (63, 64)):
            x, y, th = _straight(xs, n_traj=2)
            x[1, list(pair)] = 5.0
            r = q.query(R._params(n=n), x, y, th, want_pose_clearance=True)
            a, b = pair
            assert r.pose_clearance[1, a].view(np.uint64) == r.pose_clearance[1, b].view(np.uint64)
            assert r.min_pose[1] == min(pair) and r.min_clearance[1] == r.pose_clearance[1, a] and 0.0 < r.min_clearance[1] < 5.0
            assert r.min_pose[0] == 0 and r.min_clearance[0] > 900.0
        # trajectories with bit-equal minima: best is the smallest k; with nothing in reach every minimum is +inf and best is 0
        x, y, th = _straight([5.0, 40.0], n_traj=5, dy=0.0)
        x[0, 0] = x[3, 0] = 20.0
        r = q.query(R._params(n=2), x, y, th)
        assert r.min_clearance[1] == r.min_clearance[2] == r.min_clearance[4] < r.min_clearance[0] == r.min_clearance[3]
        assert r.best == 0 and r.first_clear == 0 and r.n_below == 0
        r = q.query(R._params(n=2), x[1:], y[1:], th[1:], margin=float(r.min_clearance[1]))
        assert r.best == 2 and r.first_clear == 2 and r.n_below == 3
        r = q.query(R._params(n=2), x, y, th, cutoff=1e-3)
        assert np.isinf(r.min_clearance).all() and r.best == 0 and r.first_clear == 0 and (r.nearest == -1).all()


def test_nothing_stale():
    """A second query on the same object after set_obstacles with other tables, and a smaller K after a larger one."""
    from commonroad_rp_amd import ClearanceQuery
    cs = R.cases()
    big, small = cs[R.DEVICE_MEMORY_CASE], cs[2]
    with ClearanceQuery(0) as q, ClearanceQuery(0) as fresh:
        q.set_obstacles(big.obs)
        first = q.query(big.p, big.x, big.y, big.th, lengths=big.lengths, want_pose_clearance=True)
        q.set_obstacles(small.obs)
        fresh.set_obstacles(small.obs)
        for obj in (q, fresh):
            r = obj.query(small.p, small.x, small.y, small.th, lengths=small.lengths, want_pose_clearance=True)
            fin = np.isfinite(small.clear)
            np.testing.assert_array_equal(np.isinf(r.pose_clearance), ~fin)
            assert np.abs(r.pose_clearance[fin] - small.clear[fin]).max() <= R.TOL
            if obj is q:
                mine = r
        for name in ("pose_clearance", "min_clearance", "min_pose", "nearest"):
            np.testing.assert_array_equal(getattr(mine, name), getattr(r, name))
        assert (mine.first_clear, mine.n_below, mine.best) == (r.first_clear, r.n_below, r.best)
        # the larger batch's own tables against the smaller batch's first trajectories, then the larger batch again
        q.set_obstacles(big.obs)
        part = q.query(big.p, big.x[:3], big.y[:3], big.th[:3], lengths=big.lengths[:3], want_pose_clearance=True)
        np.testing.assert_array_equal(part.pose_clearance, first.pose_clearance[:3])
        np.testing.assert_array_equal(part.nearest, first.nearest[:3])
        assert (part.first_clear, part.n_below, part.best) == _scalars(part.min_clearance, 0.0)
        again = q.query(big.p, big.x, big.y, big.th, lengths=big.lengths, want_pose_clearance=True)
        for name in ("pose_clearance", "min_clearance", "min_pose", "nearest"):
            np.testing.assert_array_equal(getattr(again, name), getattr(first, name))


def _raw_query(q, p, K, n, poses=None, lens=None, cutoff=INF, margin=0.0, outputs=False):
    """rp_clearance_query as a C caller makes it (the argument errors the Python interface cannot express; NULL outputs)."""
    from commonroad_rp_amd._capi import dptr
    ip = C.POINTER(C.c_int32)
    fc, nb, best = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    rc = q._lib.rp_clearance_query(q._h, C.byref(p) if p is not None else None, K, n, dptr(poses), dptr(poses), dptr(poses),
                                   lens.ctypes.data_as(ip) if lens is not None else None, cutoff, margin, None, None, None, None,
                                   C.byref(fc) if outputs else None, C.byref(nb) if outputs else None, C.byref(best) if outputs else None)
    return rc, (q._lib.rp_clearance_last_error(q._h) or b"").decode(), (fc.value, nb.value, best.value)


def test_edges_and_argument_errors():
    from commonroad_rp_amd import ClearanceQuery
    from commonroad_rp_amd._capi import RpError
    from commonroad_rp_amd.clearance import MAX_POSES
    EINVAL = -1
    c = R.cases()[R.DEVICE_MEMORY_CASE]
    p = R._params(n=4)
    z = np.zeros((3, 4))
    with ClearanceQuery(0) as q:
        # before any set_obstacles, and with empty tables: every clearance is +inf, the first trajectory is the first clear one
        for _ in range(2):
            r = q.query(c.p, c.x, c.y, c.th, lengths=c.lengths, want_pose_clearance=True)
            assert np.isinf(r.pose_clearance).all() and np.isinf(r.min_clearance).all()
            assert (r.min_pose == -1).all() and (r.nearest == -1).all() and (r.first_clear, r.n_below, r.best) == (0, 0, 0)
            q.set_obstacles(ObstacleTables())
        # K = 0
        e = np.zeros((0, 5))
        r = q.query(c.p, e, e, e, want_pose_clearance=True)
        assert (r.first_clear, r.n_below, r.best) == (-1, 0, -1) and r.min_clearance.shape == (0,) and r.pose_clearance.shape == (0, 5)
        assert _raw_query(q, p, 0, 4, None, outputs=True)[::2] == (0, (-1, 0, -1))
        # every output pointer NULL, then only the scalars
        q.set_obstacles(ObstacleTables(static_circ=[[R.WB, 0.0, 1.0]]))
        assert _raw_query(q, p, 3, 4, z)[0] == 0
        assert _raw_query(q, p, 3, 4, z, outputs=True)[::2] == (0, (-1, 3, 0))
        assert _raw_query(q, p, 3, 4, z, cutoff=5.0, margin=INF, outputs=True)[::2] == (0, (-1, 3, 0))
        for what, rc in (("K < 0", _raw_query(q, p, -1, 4, z)),
                         ("n_poses < 1", _raw_query(q, p, 3, 0, z)),
                         ("len too small", _raw_query(q, p, 3, 4, z, lens=np.array([4, 0, 1], np.int32))),
                         ("len too large", _raw_query(q, p, 3, 4, z, lens=np.array([4, 1, 5], np.int32))),
                         ("null poses", _raw_query(q, p, 3, 4, None)),
                         ("null params", _raw_query(q, None, 3, 4, z)),
                         ("beyond the pose limit", _raw_query(q, p, MAX_POSES // 4 + 1, 4, z)),
                         ("cutoff 0", _raw_query(q, p, 3, 4, z, cutoff=0.0)),
                         ("cutoff < 0", _raw_query(q, p, 3, 4, z, cutoff=-1.0)),
                         ("cutoff NaN", _raw_query(q, p, 3, 4, z, cutoff=math.nan)),
                         ("margin < 0", _raw_query(q, p, 3, 4, z, margin=-1e-9)),
                         ("margin NaN", _raw_query(q, p, 3, 4, z, margin=math.nan))):
            assert rc[0] == EINVAL and rc[1], (what, rc)
        bad = R._params(n=4)
        bad.struct_size += 8
        rc = _raw_query(q, bad, 3, 4, z)
        assert rc[0] == -7 and "struct_size" in rc[1]   # RP_EABI
        assert _raw_query(q, p, 3, 4, z, lens=np.array([4, 1, 4], np.int32), outputs=True)[::2] == (0, (-1, 3, 0))   # ... and it still works
        # through the Python interface: RpError for what the library refuses, ValueError for shapes that do not agree
        for kw in (dict(cutoff=0.0), dict(margin=-1.0), dict(lengths=[4, 4, 5]), dict(lengths=[0, 4, 4])):
            with pytest.raises(RpError, match="-> -1"):
                q.query(p, z, z, z, **kw)
        with pytest.raises(RpError, match="-> -1"):
            q.query(p, np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)))
        with pytest.raises(ValueError):
            q.query(p, z, z[:, :3], z)
        with pytest.raises(ValueError):
            q.query(p, z, z, z, lengths=[4, 4])
        q.close()
        q.close()   # (closing twice is harmless)


def test_query_states_reads_the_pose_rows():
    from commonroad_rp_amd import ClearanceQuery
    from commonroad_rp_amd.clearance import RP_N_ARRAYS, RP_THETA, RP_X, RP_Y
    c = R.cases()[0]
    n = 9
    rng = np.random.default_rng(7)
    states = rng.normal(0.0, 50.0, (3, RP_N_ARRAYS, n))        # every other row: noise the query must not read
    assert RP_N_ARRAYS == 14
    for k in range(3):
        states[k, RP_X], states[k, RP_Y], states[k, RP_THETA] = c.x[0, 40 * k:40 * k + n], c.y[0, 40 * k:40 * k + n], c.th[0, 40 * k:40 * k + n]
    p = R._params(time_step0=c.p.time_step0, factor=1, n=n)
    with ClearanceQuery(0) as q:
        q.set_obstacles(c.obs)
        a = q.query_states(p, states, lengths=[n, 4, n], cutoff=50.0, margin=R.MARGIN, want_pose_clearance=True)
        b = q.query(p, states[:, RP_X], states[:, RP_Y], states[:, RP_THETA], lengths=[n, 4, n], cutoff=50.0, margin=R.MARGIN, want_pose_clearance=True)
        for name in ("pose_clearance", "min_clearance", "min_pose", "nearest"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
        assert (a.first_clear, a.n_below, a.best) == (b.first_clear, b.n_below, b.best)
        assert np.isfinite(a.min_clearance).any() and np.isinf(a.pose_clearance[1, 4:]).all()
        with pytest.raises(ValueError):
            q.query_states(p, states[:, :3])
