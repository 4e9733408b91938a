"""Ensemble collision check (include/rp_ensemble.h, commonroad_rp_amd.ensemble_check) against the oracle: ``oracle.check_poses`` and
``oracle.check_swept`` per (trajectory, member), with tables built from that member's table, are the only source of expected values,
and every verdict -- first colliding pose and segment per member, members hit, first trajectory at or below the threshold, number
above it -- has to be EQUAL.

Shapes (tests/_ensemble.py): the smallest at which this kernel can go wrong -- a wavefront is 64 consecutive poses of one trajectory
for one block of EN_MEMBER_BLOCK members, a workgroup four wavefronts, static shapes are staged in LDS up to a capacity and read from
device memory beyond it.  The first tests run on the oracle alone: they say that the inputs can tell a wrong kernel from a right one."""
import ctypes as C

import numpy as np
import pytest

import _ensemble as E
from commonroad_rp_amd.collision import ObstacleTables
from test_trajectory_check import WB, _oracle_batch, _params

MODES = (dict(poses=True, swept=False), dict(poses=False, swept=True), dict(poses=True, swept=True))


@pytest.fixture(scope="module")
def cases():
    return E.cases()


@pytest.fixture(scope="module")
def boundary_cases():
    return E.boundary_cases()


# ---- on the oracle alone -----------------------------------------------------------------------------------------------------------
def test_oracle_verdicts_depend_on_the_member(cases):
    for idx in (E.SPREAD_5, E.SPREAD_17):
        c = cases[idx]
        assert c.M == E.CASES[idx][-1] and c.M in (5, 17)
        for kw in MODES[:2]:
            count = E.members_hit(c.first_pose, c.first_seg, **kw)
            assert int(((count > 0) & (count < c.M)).sum()) >= 5, (idx, kw, count)
    # ... some trajectory has first hits that differ between two members that both hit
    for name in ("first_pose", "first_seg"):
        differ = 0
        for c in cases:
            f = getattr(c, name)
            top = np.where(f >= 0, f, -1).max(axis=1)
            low = np.where(f >= 0, f, np.iinfo(np.int32).max).min(axis=1)
            differ += int(((f >= 0).sum(axis=1) >= 2)[top != low].sum())
        assert differ >= 1, name
    # ... trajectories free in every member and trajectories that collide in every member occur, in every mode
    for kw in MODES:
        counts = [(E.members_hit(c.first_pose, c.first_seg, **kw), c.M) for c in cases if c.M > 1]
        assert any((n == 0).any() for n, _ in counts) and any((n == M).any() for n, M in counts), kw
    # ... without dynamic obstacles a trajectory is hit in no member or in all, and both occur
    d = cases[E.NO_DYN]
    assert d.members.shape[1] == 0 and set(E.members_hit(d.first_pose, d.first_seg, True, True).tolist()) == {0, d.M}
    # ... and the threshold matters: first_free at max_members_hit = 0 and at 1 differ somewhere
    moved = 0
    for c in cases:
        count = E.members_hit(c.first_pose, c.first_seg, True, True)
        moved += E.first_free_and_n_over(count, 0)[0] != E.first_free_and_n_over(count, min(1, c.M))[0]
    assert moved >= 1


def test_oracle_member_tables_reach_both_sides_of_the_time_table(cases):
    """Time indices on both sides of the dynamic table occur in both modes (as in tests/test_trajectory_check.py), every member with
    m % 3 == 2 lacks one whole obstacle, and in the case that runs the device-memory variant verdicts hang on the members' tables."""
    for c in cases:
        n, t0, f = c.x.shape[1], c.p.time_step0, c.p.factor
        if n >= 5 and c.members.shape[1]:
            first, end = c.dyn_t0, c.dyn_t0 + c.members.shape[2]
            assert t0 < first and t0 + (n - 2) >= end and t0 + (n - 1) * f >= end
        for m in range(c.M):
            if m % 3 == 2 and c.members.shape[1]:
                assert np.isnan(c.members[m, :, :, 0]).all(axis=1).any()
    c = cases[E.DEVICE_MEMORY_CASE]
    assert len(c.obs.static_obb) + len(c.obs.static_tri) + len(c.obs.static_circ) == E.LDS_ROWS + 1 and c.p.factor == 3
    first_pose, _, first_seg = _oracle_batch(c.p, E.static_only(c.obs), c.x, c.y, c.th, c.lengths)
    assert (c.first_pose != first_pose[:, None]).any(axis=1).sum() >= 5 and (c.first_seg != first_seg[:, None]).any(axis=1).sum() >= 5


def test_oracle_first_hits_lie_on_both_sides_of_the_wavefront_boundary(boundary_cases):
    """The construction of _ensemble._boundary_scene gives what it aims at: in the n = 130 and the n = 70 scene one trajectory has
    first hits below and above index 63 | 64 in different members, for poses and for segments."""
    for c in boundary_cases:
        np.testing.assert_array_equal(c.first_pose, c.aim_pose)
        np.testing.assert_array_equal(c.first_seg, c.aim_seg)
    for c in boundary_cases[:2]:
        for f in (c.first_pose, c.first_seg):
            both = ((f >= 0) & (f <= 63)).any(axis=1) & (f >= 64).any(axis=1)
            assert both.any()
            assert {62, 63, 64} <= set(f[0].tolist())
    large = boundary_cases[0]
    assert {127, 128, 129, 5, 20} <= set(large.first_pose.ravel().tolist())
    assert (large.first_pose[4] == [64, 20, 64, 64]).all() and (large.first_seg[4] == [63, 20, 63, 63]).all()   # the static disc caps the members
    assert (large.first_pose[5] == 63).all() and (large.first_seg[5] == 62).all() and (large.first_pose[6] == -1).all()


# ---- on the device -----------------------------------------------------------------------------------------------------------------
def _assert_matches(r, c, kw, max_members_hit, cols=None):
    fp = c.first_pose if cols is None else c.first_pose[:, cols]
    fs = c.first_seg if cols is None else c.first_seg[:, cols]
    if kw["poses"]:
        np.testing.assert_array_equal(r.first_pose_hit, fp)
    else:
        assert r.first_pose_hit is None
    if kw["swept"]:
        np.testing.assert_array_equal(r.first_segment_hit, fs)
    else:
        assert r.first_segment_hit is None
    count = E.members_hit(fp, fs, **kw)
    np.testing.assert_array_equal(r.members_hit, count)
    assert (r.first_free, r.n_over) == E.first_free_and_n_over(count, max_members_hit)


@pytest.mark.gpu
def test_each_mode_and_both_in_one_call_match_the_oracle(cases, boundary_cases):
    from commonroad_rp_amd import EnsembleChecker
    with EnsembleChecker(0) as en:
        for c in list(cases) + list(boundary_cases):
            en.set_obstacles(c.obs, c.members, c.dyn_t0)
            for kw in MODES:
                for limit in sorted({0, min(1, c.M), c.M // 2, c.M}):
                    r = en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, max_members_hit=limit, **kw)
                    _assert_matches(r, c, kw, limit)
                assert (r.first_free, r.n_over) == (0, 0)   # (the last limit is M: nothing is above it)


@pytest.mark.gpu
def test_one_member_equals_the_trajectory_checker(cases, boundary_cases):
    from commonroad_rp_amd import EnsembleChecker, TrajectoryChecker
    with EnsembleChecker(0) as en, TrajectoryChecker(0) as ck:
        for c in list(cases) + list(boundary_cases):
            en.set_obstacles(c.obs)
            ck.set_obstacles(c.obs)
            for kw in MODES:
                r = en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, **kw)
                s = ck.check(c.p, c.x, c.y, c.th, lengths=c.lengths, **kw)
                K = c.x.shape[0]
                if kw["poses"]:
                    assert r.first_pose_hit.shape == (K, 1)
                    np.testing.assert_array_equal(r.first_pose_hit[:, 0], s.first_pose_hit)
                    np.testing.assert_array_equal(r.first_pose_hit[:, 0], c.first_pose[:, 0])
                if kw["swept"]:
                    assert r.first_segment_hit.shape == (K, 1)
                    np.testing.assert_array_equal(r.first_segment_hit[:, 0], s.first_segment_hit)
                    np.testing.assert_array_equal(r.first_segment_hit[:, 0], c.first_seg[:, 0])
                assert set(r.members_hit.tolist()) <= {0, 1}
                assert (r.first_free, r.n_over) == (s.first_free, s.n_hit) and int(r.members_hit.sum()) == s.n_hit


@pytest.mark.gpu
def test_member_order_permutes_the_columns(cases):
    from commonroad_rp_amd import EnsembleChecker
    with EnsembleChecker(0) as en:
        for idx in (E.SPREAD_5, E.SPREAD_17, E.N70, len(cases) - 1):
            c = cases[idx]
            perm = np.roll(np.arange(c.M)[::-1], 1)
            kw = MODES[2]
            en.set_obstacles(c.obs, c.members, c.dyn_t0)
            a = en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, max_members_hit=1, **kw)
            en.set_obstacles(c.obs, c.members[perm], c.dyn_t0)
            b = en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, max_members_hit=1, **kw)
            np.testing.assert_array_equal(b.first_pose_hit, a.first_pose_hit[:, perm])
            np.testing.assert_array_equal(b.first_segment_hit, a.first_segment_hit[:, perm])
            np.testing.assert_array_equal(b.members_hit, a.members_hit)
            assert (b.first_free, b.n_over) == (a.first_free, a.n_over)
            _assert_matches(b, c, kw, 1, cols=perm)


@pytest.mark.gpu
def test_one_object_over_several_calls(cases):
    """M = 17, then 2, then 17 with other tables, K shrinking and growing: no stale columns or rows.  set_static alone keeps the
    members, set_members alone keeps the static shapes."""
    from commonroad_rp_amd import EnsembleChecker
    from oracle import oracle  # noqa: F401  (the oracle library is what the expected values below come from)
    kw = MODES[2]
    big, small, huge = cases[E.SPREAD_17], cases[1], cases[7]
    with EnsembleChecker(0) as en:
        en.set_obstacles(big.obs, big.members, big.dyn_t0)
        _assert_matches(en.check(big.p, big.x, big.y, big.th, lengths=big.lengths, max_members_hit=3, **kw), big, kw, 3)
        en.set_obstacles(small.obs, small.members, small.dyn_t0)
        _assert_matches(en.check(small.p, small.x, small.y, small.th, lengths=small.lengths, **kw), small, kw, 0)
        rev = np.arange(big.M)[::-1]
        en.set_obstacles(big.obs, big.members[rev], big.dyn_t0)
        _assert_matches(en.check(big.p, big.x, big.y, big.th, lengths=big.lengths, max_members_hit=3, **kw), big, kw, 3, cols=rev)
        en.set_obstacles(huge.obs, huge.members, huge.dyn_t0)   # K = 257
        _assert_matches(en.check(huge.p, huge.x, huge.y, huge.th, lengths=huge.lengths, **kw), huge, kw, 0)
        # rows of a smaller call: the first 5 trajectories of the M = 17 case, lengths and all
        en.set_obstacles(big.obs, big.members, big.dyn_t0)
        r = en.check(big.p, big.x[:5], big.y[:5], big.th[:5], lengths=big.lengths[:5], max_members_hit=3, **kw)
        np.testing.assert_array_equal(r.first_pose_hit, big.first_pose[:5])
        np.testing.assert_array_equal(r.first_segment_hit, big.first_seg[:5])
        np.testing.assert_array_equal(r.members_hit, E.members_hit(big.first_pose[:5], big.first_seg[:5], True, True))
        # set_static alone: the members stay
        c = cases[E.N70]
        en.set_obstacles(c.obs, c.members, c.dyn_t0)
        _assert_matches(en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, **kw), c, kw, 0)
        en.set_static(ObstacleTables())
        bare = E.Case()
        bare.first_pose, bare.first_seg = E.oracle_ensemble(c.p, ObstacleTables(), c.members, c.dyn_t0, c.x, c.y, c.th, c.lengths)
        _assert_matches(en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, **kw), bare, kw, 0)
        en.set_static(c.obs)
        _assert_matches(en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, **kw), c, kw, 0)
        # set_members alone: the static shapes stay
        en.set_members(c.members[[5, 2]], c.dyn_t0)
        _assert_matches(en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, max_members_hit=1, **kw), c, kw, 1, cols=[5, 2])


@pytest.mark.gpu
def test_time_index_rule_per_member():
    """The scene of test_trajectory_check.py::test_time_index_rule with members and a table that covers time indices 9 .. 16 only
    (time_step0 = 7): trajectory k drives 12 m per step and has, in member m, an obstacle in the gap between poses 4 and 5 at ONE time
    index, time_step0 + 4 + shift(k, m): swept sees it in segment 4 where the shift is 0, whatever the factor.  An obstacle ON pose 3
    at index 16 only: the per-pose test meets it with factor 3 and not with factor 1.  An obstacle on pose 0 and one on pose 11 in
    every row of the table: their time indices lie before and behind the table, nothing meets them.  Member 2 is all NaN.
    Trajectory 0 has a static disc on pose 6 besides: the only verdict of member 2, a cap for the others."""
    from commonroad_rp_amd import EnsembleChecker
    K, n, t0, M, dyn_t0, n_steps = 65, 12, 7, 4, 9, 8
    x = np.tile(12.0 * np.arange(n), (K, 1))
    y = np.tile(100.0 * np.arange(K)[:, None], (1, n))
    th = np.zeros((K, n))
    shift = (np.arange(K)[:, None] + np.arange(M)[None, :]) % 5 - 2
    gap_x = 0.5 * (x[0, 4] + x[0, 5]) + WB
    members = np.full((M, 4 * K, n_steps, 5), np.nan)
    for m in range(M):
        if m == 2:
            continue
        for k in range(K):
            members[m, k, t0 + 4 + shift[k, m] - dyn_t0] = (gap_x, y[k, 0], 0.0, 0.3, 0.3)
            members[m, K + k, t0 + 3 * 3 - dyn_t0] = (x[k, 3] + WB, y[k, 0], 0.0, 0.3, 0.3)
            members[m, 2 * K + k, :] = (x[k, 0] + WB, y[k, 0], 0.0, 0.3, 0.3)
            members[m, 3 * K + k, :] = (x[k, 11] + WB, y[k, 0], 0.0, 0.3, 0.3)
    obs = ObstacleTables(static_circ=[[x[0, 6] + WB, y[0, 0], 0.2]], dyn_obb=members[0], dyn_t0=dyn_t0)
    live = np.array([m != 2 for m in range(M)])
    with EnsembleChecker(0) as en:
        en.set_obstacles(obs, members, dyn_t0)
        for factor in (1, 3):
            p = _params(time_step0=t0, factor=factor, n=n)
            want_pose, want_seg = E.oracle_ensemble(p, obs, members, dyn_t0, x, y, th, None)
            # (the oracle says what the rule says)
            np.testing.assert_array_equal(want_seg[1:], np.where((shift[1:] == 0) & live, 4, -1))
            np.testing.assert_array_equal(want_pose[1:], np.where(live, 3 if factor == 3 else -1, -1) * np.ones((K - 1, 1), int))
            np.testing.assert_array_equal(want_pose[0], np.where(live, 3 if factor == 3 else 6, 6))
            np.testing.assert_array_equal(want_seg[0], np.where((shift[0] == 0) & live, 4, 5))
            r = en.check(p, x, y, th, poses=True, swept=True, max_members_hit=1)
            np.testing.assert_array_equal(r.first_pose_hit, want_pose)
            np.testing.assert_array_equal(r.first_segment_hit, want_seg)
            count = E.members_hit(want_pose, want_seg, True, True)
            np.testing.assert_array_equal(r.members_hit, count)
            assert (r.first_free, r.n_over) == E.first_free_and_n_over(count, 1)
            assert r.members_hit[0] == M and (r.members_hit[1:] == (3 if factor == 3 else (shift[1:] == 0)[:, live].sum(axis=1))).all()


def _raw_check(en, p, mode, K, n, poses=None, lens=None, max_hit=0, first_pose=None, first_seg=None, members_hit=None, want_ff=True,
               want_no=True):
    """rp_ensemble_check as a C caller makes it: return code, message, first_free, n_over (7 where the call left them alone)."""
    from commonroad_rp_amd._capi import dptr
    ip = C.POINTER(C.c_int32)
    as_ip = lambda a: a.ctypes.data_as(ip) if a is not None else None   # noqa: E731
    ff, no = C.c_int64(7), C.c_int64(7)
    rc = en._lib.rp_ensemble_check(en._h, C.byref(p) if p is not None else None, mode, K, n, dptr(poses), dptr(poses), dptr(poses), as_ip(lens),
                                   max_hit, as_ip(first_pose), as_ip(first_seg), as_ip(members_hit), C.byref(ff) if want_ff else None,
                                   C.byref(no) if want_no else None)
    return rc, (en._lib.rp_ensemble_last_error(en._h) or b"").decode(), ff.value, no.value


@pytest.mark.gpu
def test_edges(cases):
    from commonroad_rp_amd import EnsembleChecker
    from commonroad_rp_amd._capi import dptr
    from commonroad_rp_amd.ensemble_check import TRAJ_POSES, TRAJ_SWEPT
    kw = MODES[2]
    c = cases[E.DEVICE_MEMORY_CASE]
    with EnsembleChecker(0) as en:
        # a fresh object: no static shapes, one member without dynamic obstacles
        r = en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, **kw)
        assert r.first_pose_hit.shape == (len(c.x), 1) and (r.first_pose_hit == -1).all() and (r.first_segment_hit == -1).all()
        assert (r.members_hit == 0).all() and (r.first_free, r.n_over) == (0, 0)
        # K = 0
        en.set_obstacles(c.obs, c.members, c.dyn_t0)
        e = np.zeros((0, 5))
        r = en.check(c.p, e, e, e, max_members_hit=2, **kw)
        assert (r.first_free, r.n_over) == (-1, 0) and r.first_pose_hit.shape == (0, c.M) and r.members_hit.shape == (0,)
        # n_dyn = 0 with M = 4 and with M = 3: a verdict comes from the static shapes, so it is the same in every member
        d = cases[E.NO_DYN]
        assert d.members.shape[1] == 0
        for members in (d.members, d.members[:3]):
            M = members.shape[0]
            en.set_obstacles(d.obs, members, d.dyn_t0)
            r = en.check(d.p, d.x, d.y, d.th, lengths=d.lengths, max_members_hit=M - 1, **kw)
            _assert_matches(r, d, kw, M - 1, cols=list(range(M)))
            assert set(r.members_hit.tolist()) <= {0, M}
        # len[k] = 1: no segment, in any member; the ragged cases end in such a trajectory
        en.set_obstacles(c.obs, c.members, c.dyn_t0)
        ones = np.ones(len(c.x), np.int32)
        r = en.check(c.p, c.x, c.y, c.th, lengths=ones, **kw)
        assert (r.first_segment_hit == -1).all()
        np.testing.assert_array_equal(r.first_pose_hit, np.where(c.first_pose == 0, 0, -1))
        assert c.lengths[-1] == 1 and (c.first_seg[-1] == -1).all()
        # every output pointer NULL except one, each in turn
        K, n, M = c.x.shape[0], c.x.shape[1], c.M
        count = E.members_hit(c.first_pose, c.first_seg, True, True)
        lens = np.ascontiguousarray(c.lengths, np.int32)

        def call(**out):
            ip = C.POINTER(C.c_int32)
            a = {name: (v.ctypes.data_as(ip) if isinstance(v, np.ndarray) else C.byref(v)) for name, v in out.items()}
            rc = en._lib.rp_ensemble_check(en._h, C.byref(c.p), TRAJ_POSES | TRAJ_SWEPT, K, n, dptr(c.x), dptr(c.y), dptr(c.th), lens.ctypes.data_as(ip),
                                           2, a.get("first_pose"), a.get("first_seg"), a.get("members_hit"), a.get("first_free"), a.get("n_over"))
            assert rc == 0, (rc, en._lib.rp_ensemble_last_error(en._h))
        call()
        buf = np.full((K, M), 99, np.int32)
        call(first_pose=buf)
        np.testing.assert_array_equal(buf, c.first_pose)
        buf = np.full((K, M), 99, np.int32)
        call(first_seg=buf)
        np.testing.assert_array_equal(buf, c.first_seg)
        buf = np.full(K, 99, np.int32)
        call(members_hit=buf)
        np.testing.assert_array_equal(buf, count)
        v = C.c_int64(99)
        call(first_free=v)
        assert v.value == E.first_free_and_n_over(count, 2)[0]
        v = C.c_int64(99)
        call(n_over=v)
        assert v.value == E.first_free_and_n_over(count, 2)[1]
    en.close()   # (closing twice is harmless)


@pytest.mark.gpu
def test_argument_errors(cases):
    """Every refusal comes from the host, before anything is launched, and the object gives correct results afterwards."""
    from commonroad_rp_amd import EnsembleChecker
    from commonroad_rp_amd._capi import RpError, dptr
    from commonroad_rp_amd.ensemble_check import MAX_DYN_ROWS, MAX_MEMBERS, MAX_POSES, MAX_VERDICTS, TRAJ_POSES, TRAJ_SWEPT
    EINVAL, EABI = -1, -7
    c = cases[E.SPREAD_17]
    kw = MODES[2]
    p = _params(n=4)
    z = np.zeros((3, 4))
    i3m = np.zeros((3, c.M), np.int32)
    with EnsembleChecker(0) as en:
        en.set_obstacles(c.obs, c.members, c.dyn_t0)
        M = c.M
        assert _raw_check(en, p, TRAJ_POSES | TRAJ_SWEPT, 3, 4, z)[0] == 0
        many = np.zeros(MAX_VERDICTS // M + 1)   # (as many trajectories of one pose: within the pose limit, beyond the verdict limit)
        for what, rc in (("no mode bit", _raw_check(en, p, 0, 3, 4, z)),
                         ("unknown mode bit", _raw_check(en, p, TRAJ_POSES | 4, 3, 4, z)),
                         ("K < 0", _raw_check(en, p, TRAJ_POSES, -1, 4, z)),
                         ("n_poses < 1", _raw_check(en, p, TRAJ_POSES, 3, 0, z)),
                         ("len too small", _raw_check(en, p, TRAJ_POSES, 3, 4, z, lens=np.array([4, 0, 1], np.int32))),
                         ("len too large", _raw_check(en, p, TRAJ_POSES, 3, 4, z, lens=np.array([4, 1, 5], np.int32))),
                         ("first_pose_hit without POSES", _raw_check(en, p, TRAJ_SWEPT, 3, 4, z, first_pose=i3m)),
                         ("first_segment_hit without SWEPT", _raw_check(en, p, TRAJ_POSES, 3, 4, z, first_seg=i3m)),
                         ("null poses", _raw_check(en, p, TRAJ_POSES, 3, 4, None)),
                         ("null params", _raw_check(en, None, TRAJ_POSES, 3, 4, z)),
                         ("max_members_hit < 0", _raw_check(en, p, TRAJ_POSES, 3, 4, z, max_hit=-1)),
                         ("max_members_hit > n_members", _raw_check(en, p, TRAJ_POSES, 3, 4, z, max_hit=M + 1)),
                         ("max_members_hit > n_members, K = 0", _raw_check(en, p, TRAJ_POSES, 0, 4, z, max_hit=M + 1)),
                         ("beyond the pose limit", _raw_check(en, p, TRAJ_POSES, MAX_POSES // 4 + 1, 4, z)),
                         ("beyond the verdict limit", _raw_check(en, p, TRAJ_POSES, len(many), 1, many))):
            assert rc[0] == EINVAL and rc[1] and rc[2:] == (7, 7), (what, rc)
        assert _raw_check(en, p, TRAJ_POSES, 3, 4, z, max_hit=M)[0] == 0
        old = type(p).from_buffer_copy(p)
        old.struct_size -= 8
        rc = _raw_check(en, old, TRAJ_POSES, 3, 4, z)
        assert rc[0] == EABI and rc[1] and rc[2:] == (7, 7)
        # the tables: a refused call leaves the earlier ones in place
        lib, h = en._lib, en._h
        one = np.zeros(5)
        for what, rc in (("n_members = 0", lib.rp_ensemble_set_members(h, 0, 1, 1, 0, dptr(one))),
                         ("n_members beyond the limit", lib.rp_ensemble_set_members(h, MAX_MEMBERS + 1, 0, 0, 0, None)),
                         ("n_dyn < 0", lib.rp_ensemble_set_members(h, 1, -1, 1, 0, dptr(one))),
                         ("n_steps < 0", lib.rp_ensemble_set_members(h, 1, 1, -1, 0, dptr(one))),
                         ("rows beyond the limit", lib.rp_ensemble_set_members(h, MAX_MEMBERS, MAX_DYN_ROWS // MAX_MEMBERS + 1, 1, 0, dptr(one))),
                         ("rows beyond the limit, large counts", lib.rp_ensemble_set_members(h, 2, 2**31 - 1, 2**31 - 1, 0, dptr(one))),
                         ("null table with rows", lib.rp_ensemble_set_members(h, 2, 1, 1, 0, None)),
                         ("negative static count", lib.rp_ensemble_set_static(h, -1, None, 0, None, 0, None)),
                         ("null static table", lib.rp_ensemble_set_static(h, 0, None, 2, None, 0, None))):
            assert rc == EINVAL and lib.rp_ensemble_last_error(h), what
        # through the Python interface: RpError for what the library refuses, ValueError for shapes that do not agree
        for bad in (dict(poses=False, swept=False), dict(lengths=[4, 4, 5]), dict(lengths=[0, 4, 4]), dict(max_members_hit=M + 1),
                    dict(max_members_hit=-1)):
            with pytest.raises(RpError, match="-> -1"):
                en.check(p, z, z, z, **bad)
        with pytest.raises(RpError, match="-> -1"):
            en.check(p, np.zeros((2, 0)), np.zeros((2, 0)), np.zeros((2, 0)))
        with pytest.raises(ValueError):
            en.check(p, z, z[:, :3], z)
        with pytest.raises(ValueError):
            en.check(p, z, z, z, lengths=[4, 4])
        with pytest.raises(ValueError):
            en.set_members(np.zeros((2, 3, 4)))
        # ... and the object still holds its tables and works
        _assert_matches(en.check(c.p, c.x, c.y, c.th, lengths=c.lengths, max_members_hit=2, **kw), c, kw, 2)
