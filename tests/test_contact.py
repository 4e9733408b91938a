"""Collision verdicts of the HIP paths at near contact against the exact reference of tests/_contact.py: about four thousand
configurations -- touching edges, corners, diagonals in line, strips touched at their far end, degenerate triangles, point circles,
swept boxes -- a few B = 8 u scale to a micrometre on either side of contact, at the origin and up to three thousand kilometres out.
The reference decides every one of them (tests/test_contact_abi.py); a verdict here is right or wrong, there is no tolerance.

librp_check, librp_ensemble and librp_clearance take the whole table in a handful of launches each (the packing is described in
tests/_contact.py); rp_check_swept takes one case per call; rp_plan gets obstacles placed against poses of the extended-precision
rows of tests/_xref.py, on four launch paths in production and draw mode; a few rectangles touch exactly (g = 0: a hit).
What is compared where: the ragged batches (1 x 130, 65 x 63) show the POSE FLAG of every case, and first_pose_hit /
first_segment_hit of a trajectory's first overlapping case only; every case's own first_pose_hit and first_segment_hit come from
one trajectory per case -- dynamic cases in the same scene as the ragged batch, static cases as trajectories of two poses.  Not
shown: first_segment_hit along a trajectory that visits several static cases (the long box between two of them holds both ego
rectangles and is as close to their obstacles)."""
import numpy as np
import pytest

import _contact as C
from commonroad_rp_amd.collision import ObstacleTables

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not C.HAVE_LONGDOUBLE, reason=C.SKIP_REASON)]


@pytest.fixture(scope="module")
def T():
    return C.table()


def _wrong(T, cases, got, want):
    bad = cases[(got != want) & (cases >= 0)]
    return [(str(T.name[i]), int(T.oi[i]), int(T.hi[i]), int(T.dk[i]), int(T.sign[i]), f"g = {float(T.g[i]):.3e} = {float(T.g[i]) / T.B[i]:.1f} B") for i in bad[:12]]


# ---- librp_check -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker():
    from commonroad_rp_amd.trajectory_check import TrajectoryChecker
    with TrajectoryChecker(0) as ck:
        yield ck


def _check_batch(T, ck, b, swept=True):
    ck.set_obstacles(b.obstacles)
    K, n = b.x.shape
    r = ck.check(C.params(n=n), b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=swept, want_pose_hits=True)
    ph, fp, fs = b.expected(T)
    assert not _wrong(T, b.case, r.pose_hits, ph)
    assert np.array_equal(r.pose_hits, ph)
    assert np.array_equal(r.first_pose_hit, fp)
    if swept:
        assert np.array_equal(r.first_segment_hit, fs), [(k, int(r.first_segment_hit[k]), int(fs[k])) for k in np.flatnonzero(r.first_segment_hit != fs)[:10]]
    return r


def test_checker_one_trajectory_of_130_poses(T, checker):
    b = C.single_batch(T, 130)
    assert b.x.shape == (1, 130) and (b.case >= 0).sum() == 65 and len({T.family[i] for i in b.case[b.case >= 0]}) >= 6
    _check_batch(T, checker, b)


@pytest.mark.parametrize("origin", range(len(C.ORIGINS)))
def test_checker_ragged_batch_of_an_origin(T, checker, origin):
    b = C.dynamic_batch(T, origin)
    assert b.x.shape == (C.TRAJS, C.POSES) and len(set(b.lengths)) > 2 and (b.lengths % 2).any()
    assert set(b.case[b.case >= 0]) == set(T.select(static=False, scene=origin))
    r = _check_batch(T, checker, b)
    # every trajectory holds hits: its first hits are those of its first overlapping case
    assert np.all(r.first_pose_hit >= 0)


@pytest.mark.parametrize("origin", range(len(C.ORIGINS)))
def test_checker_one_trajectory_per_dynamic_case(T, checker, origin):
    """first_pose_hit and first_segment_hit of EVERY dynamic case (family i: the merged box of two different poses against the dynamic
    walk): in the ragged batch a trajectory shows them for its first overlapping case only."""
    b = C.case_batch(T, origin)
    cases = b.case.max(axis=1)
    assert np.array_equal(np.sort(cases), T.select(static=False, scene=origin)) and ((b.case >= 0).sum(axis=1) == 1).all()
    assert np.array_equal(b.lengths, b.case.argmax(axis=1) + 2)
    checker.set_obstacles(b.obstacles)
    r = checker.check(C.params(n=b.x.shape[1]), b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=True, want_pose_hits=True)
    ph, fp, fs = b.expected(T)
    assert not _wrong(T, cases, r.first_segment_hit, fs) and not _wrong(T, cases, r.first_pose_hit, fp)
    assert np.array_equal(r.first_segment_hit, fs) and np.array_equal(r.first_pose_hit, fp) and np.array_equal(r.pose_hits, ph)
    hit = T.hit[cases]
    for f in ("a", "b", "c", "d", "f", "i"):     # both verdicts of every family are seen ("e": containment, hits alone)
        assert hit[T.family[cases] == f].any() and (~hit[T.family[cases] == f]).any(), f
    assert set(T.branch[cases[T.swept[cases]]]) == {0, 1, 2}


@pytest.mark.parametrize("variant", ["lds", "device_memory"])
def test_checker_static_scenes(T, checker, variant):
    seen = 0
    for scene in range(T.n_static_scenes):
        n_static = len(T.select(static=True, scene=scene))
        pad = C.LDS_ROWS + 1 - n_static if variant == "device_memory" else 0
        poses, swept = C.static_batches(T, scene, pad_static=pad)
        total = len(poses.obstacles.static_obb) + len(poses.obstacles.static_tri) + len(poses.obstacles.static_circ)
        assert total == (C.LDS_ROWS + 1 if pad else n_static) and n_static <= C.LDS_ROWS
        _check_batch(T, checker, poses, swept=False)
        _check_batch(T, checker, swept)
        seen += n_static
    assert seen == int(T.static.sum())


# ---- librp_ensemble --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ensemble():
    from commonroad_rp_amd.ensemble_check import EnsembleChecker
    with EnsembleChecker(0) as en:
        yield en


@pytest.mark.parametrize("origin", range(len(C.ORIGINS)))
def test_ensemble_plus_and_minus_are_two_members(T, ensemble, origin):
    b = C.member_batch(T, origin)
    K, n = b.x.shape
    ensemble.set_obstacles(ObstacleTables(), members=b.members, dyn_t0=0)
    r = ensemble.check(C.params(n=n), b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=True)
    at = b.case.max(axis=2)                       # [2, K]: the case of member m in trajectory k
    where = b.case.argmax(axis=2)                 # and its pose
    want_pose = np.where(T.hit_pose[at], where, -1).T
    want_seg = np.where(T.hit[at], where, -1).T
    for m in range(2):
        assert not _wrong(T, at[m], r.first_pose_hit[:, m], want_pose[:, m])
        assert not _wrong(T, at[m], r.first_segment_hit[:, m], want_seg[:, m])
    assert np.array_equal(r.first_pose_hit, want_pose) and np.array_equal(r.first_segment_hit, want_seg)
    assert np.array_equal(r.members_hit, ((want_pose >= 0) | (want_seg >= 0)).sum(1))
    assert set(r.members_hit) == {1, 2}           # (2: containment, the same shape in both members)


def test_ensemble_static_scenes(T, ensemble):
    for scene in range(T.n_static_scenes):
        for b in C.static_batches(T, scene):
            ensemble.set_obstacles(b.obstacles)
            K, n = b.x.shape
            r = ensemble.check(C.params(n=n), b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=n == 2)
            ph, fp, fs = b.expected(T)
            assert np.array_equal(r.first_pose_hit[:, 0], fp), _wrong(T, b.case[:, 0], r.first_pose_hit[:, 0], fp)
            if n == 2:
                assert np.array_equal(r.first_segment_hit[:, 0], fs), _wrong(T, b.seg_case[:, 0], r.first_segment_hit[:, 0], fs)
                assert np.array_equal(r.members_hit, ((fp >= 0) | (fs >= 0)).astype(np.int32))


# ---- librp_clearance -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clearance():
    from commonroad_rp_amd.clearance import ClearanceQuery
    with ClearanceQuery(0) as q:
        yield q


def _clearance_is_right(T, cases, got):
    """0.0 exactly where the sets meet, positive and within B of the exact distance elsewhere"""
    hit = T.hit_pose[cases]
    assert np.array_equal(got == 0.0, hit), _wrong(T, cases, got == 0.0, hit)
    err = np.abs(got - np.asarray(T.dist[cases], float))
    over = np.flatnonzero(~hit & ~(err <= T.B_pose[cases]))
    print(f"clearance: worst |c - exact| / B = {(err / T.B_pose[cases])[~hit].max():.3f} over {int((~hit).sum())} free cases")
    assert not len(over), [(str(T.name[cases[q]]), int(T.oi[cases[q]]), float(err[q] / T.B_pose[cases[q]])) for q in over[:10]]
    assert np.all(got[~hit] > 0.0)


def test_clearance_static_scenes(T, clearance):
    for scene in range(T.n_static_scenes):
        idx = T.select(static=True, scene=scene)
        obs = C.static_batches(T, scene)[0].obstacles
        clearance.set_obstacles(obs)
        r = clearance.query(C.params(n=1), T.a[idx, 0:1], T.a[idx, 1:2], T.a[idx, 2:3], want_pose_clearance=True)
        _clearance_is_right(T, idx, r.pose_clearance[:, 0])
        ids = C.static_ids(T, idx)
        assert np.array_equal(r.nearest, [ids[i] for i in idx])
        assert np.array_equal(r.min_clearance, r.pose_clearance[:, 0])


@pytest.mark.parametrize("origin", range(len(C.ORIGINS)))
def test_clearance_ragged_batch_of_an_origin(T, clearance, origin):
    b = C.dynamic_batch(T, origin)
    idx = T.select(static=False, scene=origin)
    clearance.set_obstacles(b.obstacles)
    K, n = b.x.shape
    r = clearance.query(C.params(n=n), b.x, b.y, b.th, lengths=b.lengths, want_pose_clearance=True)
    asked = b.case >= 0
    _clearance_is_right(T, b.case[asked], r.pose_clearance[asked])
    odd = (np.arange(n) % 2 == 1)[None, :] | (np.arange(n)[None, :] >= b.lengths[:, None])
    assert np.all(np.isinf(r.pose_clearance[odd]))             # (nothing is present at the odd time indices, nothing asked behind the end)
    assert np.all(r.pose_clearance[~asked & ~odd] > C.FOREIGN)  # (the closing pose of an odd length sees the other trajectories' shapes)
    # the trajectory's own answer: its first overlapping case, and that case's obstacle
    ph, fp, _ = b.expected(T)
    assert np.array_equal(r.min_pose, fp) and np.all(r.min_clearance == 0.0)
    assert np.array_equal(r.nearest, np.searchsorted(idx, b.case[np.arange(K), fp]))


# ---- rp_check_swept: one call per case -------------------------------------------------------------------------------------------
def test_check_swept_one_case_per_call(T):
    from commonroad_rp_amd._capi import RpContext
    picks = list(np.flatnonzero(T.swept))
    for vi, v in enumerate(C.VARIANTS):     # every other variant at every origin, both sides of contact, dynamic and static where both exist
        if v.second is None:
            for oi in range(len(C.ORIGINS)):
                for static in (False, True):
                    m = T.select(vid=vi, oi=oi, static=static)
                    if len(m):
                        first = m[T.slot[m] == T.slot[m[(vi + oi) % len(m)]]]
                        picks += [int(i) for i in first]
    ctx = RpContext(0)
    s = np.arange(0.0, 8.0, 1.0)
    ctx.set_reference(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0)
    p = C.params(n=2)
    got = np.zeros(len(picks), bool)
    for q, i in enumerate(picks):
        ctx.set_obstacles(C.single_tables(T, i))
        got[q] = ctx.check_swept(p, [T.a[i, 0], T.b[i, 0]], [T.a[i, 1], T.b[i, 1]], [T.a[i, 2], T.b[i, 2]]) == 0
    ctx.close()
    picks = np.array(picks)
    assert not _wrong(T, picks, got, T.hit[picks])
    assert set(T.branch[picks[:int(T.swept.sum())]]) == {0, 1, 2}


# ---- planner labels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["production", "draw"])
@pytest.mark.parametrize("path", C.PLANNER_PATHS)
def test_planner_labels_at_near_contact(path, mode):
    """rp_plan on three of tests/_xref.py's cases with one obstacle 1e-8 or 1e-6 m on either side of contact with a chosen (candidate,
    step) pose of the extended-precision reference: status & 3 is 3 or 1 as the reference says for every decided candidate (its smallest
    gap over all steps and shapes at least 1e-9 m from contact: the rows' allowance of 1.2e-11 m is 800 times below the displacement)."""
    import _xref as X
    from _paths import LAUNCH_PATHS, launch_path_env
    from commonroad_rp_amd._capi import RpContext
    seen, wrong = {}, []
    with launch_path_env(path):
        ctx = RpContext(0)
        try:
            for name in C.PLANNER_CASES:
                for s, lab, n_collision, how, launch in C.planner_run(ctx, name, mode == "draw"):
                    if X.forced_launch_differences(LAUNCH_PATHS[path], launch):
                        wrong.append((name, s.form, "launch", launch))
                    seen.setdefault(s.form, set()).add(how)
                    feasible = s.label != 0
                    for k in np.flatnonzero(s.decided & (lab != s.label)):
                        wrong.append((name, s.form, s.variant, s.gap, int(k), int(lab[k]), int(s.label[k]), float(s.gmin[k])))
                    if (lab[~feasible] == 3).any():
                        wrong.append((name, s.form, s.gap, "a candidate that is not feasible is labelled colliding"))
                    sure = int((s.decided & (s.label == 3)).sum())
                    if not sure <= n_collision <= sure + int((feasible & ~s.decided).sum()):
                        wrong.append((name, s.form, s.variant, s.gap, "n_collision", n_collision, "decided colliding", sure))
        finally:
            ctx.close()
    print(path, mode, {f: sorted(v) for f, v in seen.items()})
    assert not wrong, wrong[:12]
    # both instances of the query ran: the folded view (level 1, a folded table was built) and the tables as uploaded (level 2)
    assert {q[0] for q in seen["folded"]} == {1} and all(q[1] for q in seen["folded"])
    assert {q[0] for q in seen["unfolded"]} == {2} and not any(q[1] for q in seen["unfolded"])
    assert {q[0] for f in ("grid_of_five", "triangle", "circle") for q in seen[f]} == {2}
    # ... and the path's own kernel: one launch on "single_launch", two on the others, 32 / 64 lanes where the path forces them
    assert {q[3] for v in seen.values() for q in v} == {1 if path == "single_launch" else 0}
    if path in ("g32", "g64"):
        assert {q[2] for v in seen.values() for q in v} == {int(path[1:])}


# ---- exactly touching ------------------------------------------------------------------------------------------------------------
def test_exactly_touching_rectangles_collide(checker, ensemble, clearance):
    """g = 0, exactly, in the reference and in the formulas' own double arithmetic: a hit on every path (`>=` for `>` in a separating
    axis test loses these and nothing else)."""
    from commonroad_rp_amd._capi import RpContext
    ex, ey, rows = C.exact_cases()
    p, m = C.exact_params(n=2), len(ex)
    x, y, th = np.stack((ex, ex), 1), np.stack((ey, ey), 1), np.zeros((m, 2))
    dyn = np.full((m, 2, 5), np.nan)
    dyn[:, 0] = rows
    for obs in (ObstacleTables(static_obb=rows), ObstacleTables(dyn_obb=dyn, dyn_t0=0)):
        static = len(obs.static_obb) > 0
        checker.set_obstacles(obs)
        r = checker.check(p, x, y, th, poses=True, swept=True, want_pose_hits=True)
        assert np.array_equal(r.pose_hits, np.stack((np.ones(m, bool), np.full(m, static)), 1))
        assert np.all(r.first_pose_hit == 0) and np.all(r.first_segment_hit == 0)
        ensemble.set_obstacles(obs)
        r = ensemble.check(p, x, y, th, poses=True, swept=True)
        assert np.all(r.first_pose_hit == 0) and np.all(r.first_segment_hit == 0) and np.all(r.members_hit == 1)
        clearance.set_obstacles(obs)
        r = clearance.query(p, x, y, th, want_pose_clearance=True)
        assert np.all(r.pose_clearance[:, 0] == 0.0) and np.array_equal(r.nearest, np.arange(m))
    ctx = RpContext(0)
    s = np.arange(0.0, 8.0, 1.0)
    ctx.set_reference(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0)
    for k in range(m):
        for obs in (ObstacleTables(static_obb=rows[k:k + 1]), ObstacleTables(dyn_obb=dyn[k:k + 1], dyn_t0=0)):
            ctx.set_obstacles(obs)
            assert ctx.check_swept(p, x[k], y[k], th[k]) == 0, (k, rows[k])
    ctx.close()
