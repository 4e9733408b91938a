"""The near-contact case table and its exact reference (tests/_contact.py), on the CPU: the double-word gaps against mpmath at 50
digits, every case decided, the double oracle right on every case, tests/_clearance.py's distance inside the band, and planted
defects -- Python restatements of the predicate with one thing wrong -- each turning its family red."""
import os
import re

import numpy as np
import pytest

import _contact as C

pytestmark = pytest.mark.skipif(not C.HAVE_LONGDOUBLE, reason=C.SKIP_REASON)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    return C.table()


def test_lds_capacity_is_the_sources():
    src = open(os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_check.hip")).read()
    assert int(re.search(r"CK_LDS_ROWS\s*=\s*(\d+)", src).group(1)) == C.LDS_ROWS


def test_table_shape_and_grid(T):
    assert 3500 <= len(T) <= 4500
    for f in C.FAMILIES:
        m = T.family == f
        assert set(T.oi[m]) == set(range(len(C.ORIGINS))) and set(T.hi[m]) == set(range(len(C.HEADINGS))), f
        if f != "e":
            assert set(T.dk[m]) == {0, 1, 2} and set(T.sign[m]) == {1, -1}, f
    assert set(T.branch[T.swept]) == {0, 1, 2}
    for name in ("f_end_on_diagonal", "f_end_on_diagonal_hw0", "f_far_end_normal_on_diagonal", "c_front_left", "d_square", "a_segment_parallel",
                 "g_collinear_end", "g_edge_through_corner_clockwise", "g_100m_edge", "h_point_on_corner"):
        assert (T.name == name).sum() >= 2 * len(C.ORIGINS) * len(C.HEADINGS), name
    # family c: the bounding circles touch -- the centre distance is ego_r + r_bound to the displacement
    m = np.flatnonzero((T.family == "c") & ~T.static)
    cx, cy = T.a[m, 0] + C.WB * np.cos(T.a[m, 2]), T.a[m, 1] + C.WB * np.sin(T.a[m, 2])
    excess = np.hypot(T.row[m, 0] - cx, T.row[m, 1] - cy) - (C.EGO_R + np.hypot(T.row[m, 3], T.row[m, 4]))
    assert np.all(np.abs(excess) <= 1.1 * np.maximum(65536 * T.B[m], 1e-6))
    # family f, strip end on the diagonal: the ego's centre is hl + ego_r along the strip's axis (the slab test's own limit)
    m = np.flatnonzero(np.isin(T.name, ("f_end_on_diagonal", "f_end_on_diagonal_hw0")))
    cx, cy = T.a[m, 0] + C.WB * np.cos(T.a[m, 2]), T.a[m, 1] + C.WB * np.sin(T.a[m, 2])
    along = np.abs((cx - T.row[m, 0]) * np.cos(T.row[m, 2]) + (cy - T.row[m, 1]) * np.sin(T.row[m, 2]))
    assert np.all(np.abs(along - (40.0 + C.EGO_R)) <= 1.1 * np.maximum(65536 * T.B[m], 1e-6))


def test_every_case_is_decided(T):
    g, gp = np.asarray(T.g, float), np.asarray(T.g_pose, float)
    assert np.all(np.abs(g) >= C.DECIDED * T.B) and np.all(np.abs(gp) >= C.DECIDED * T.B_pose)
    assert np.all(T.hit == (T.sign <= 0))
    assert np.all(T.hit[T.family == "e"])
    # B at these coordinates: 2.7e-14 m at the origin, 4.6e-9 m three thousand kilometres out
    assert T.B.min() < 5e-14 and 3e-9 < T.B.max() < 6e-9


# ---- mpmath at 50 digits: a third statement of the same sets, scalar -------------------------------------------------------------
def _mp_case(mp, T, i):
    f = lambda v: mp.mpf(float(v))   # noqa: E731

    def ego(p):
        c, s = mp.cos(f(p[2])), mp.sin(f(p[2]))
        return [f(p[0]) + f(C.WB) * c, f(p[1]) + f(C.WB) * s, c, s, f(C.HL), f(C.HW)]

    def merge(a, b):
        dx, dy = b[0] - a[0], b[1] - a[1]
        lim = 2 * (max(a[4], a[5]) + max(b[4], b[5]))
        if mp.sqrt(dx * dx + dy * dy) > lim:
            nx, ny = dx, dy
        else:
            sg = -1 if a[2] * b[2] + a[3] * b[3] < 0 else 1
            nx, ny = a[2] + sg * b[2], a[3] + sg * b[3]
        nrm = mp.sqrt(nx * nx + ny * ny)
        nx, ny = nx / nrm, ny / nrm
        lo, hi = [], []
        for ex, ey in ((nx, ny), (-ny, nx)):
            ea = a[4] * abs(a[2] * ex + a[3] * ey) + a[5] * abs(a[3] * ex - a[2] * ey)
            eb = b[4] * abs(b[2] * ex + b[3] * ey) + b[5] * abs(b[3] * ex - b[2] * ey)
            pb = dx * ex + dy * ey
            lo.append(min(-ea, pb - eb))
            hi.append(max(ea, pb + eb))
        c0, c1 = (lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2
        return [a[0] + c0 * nx - c1 * ny, a[1] + c0 * ny + c1 * nx, nx, ny, (hi[0] - lo[0]) / 2, (hi[1] - lo[1]) / 2]

    def reach(b, nx, ny):
        return b[4] * abs(b[2] * nx + b[3] * ny) + b[5] * abs(b[2] * ny - b[3] * nx)

    def gap(e):
        r = T.row[i]
        if T.kind[i] == "rect":
            o = [f(r[0]), f(r[1]), mp.cos(f(r[2])), mp.sin(f(r[2])), f(r[3]), f(r[4])]
            tx, ty = o[0] - e[0], o[1] - e[1]
            return max(abs(tx * nx + ty * ny) - reach(e, nx, ny) - reach(o, nx, ny)
                       for nx, ny in ((e[2], e[3]), (-e[3], e[2]), (o[2], o[3]), (-o[3], o[2])))
        if T.kind[i] == "circ":
            qx, qy = f(r[0]) - e[0], f(r[1]) - e[1]
            ax, ay = abs(qx * e[2] + qy * e[3]) - e[4], abs(qy * e[2] - qx * e[3]) - e[5]
            return (mp.sqrt(max(ax, 0) ** 2 + max(ay, 0) ** 2) if ax > 0 or ay > 0 else max(ax, ay)) - f(r[2])
        v = [(f(r[2 * k]) - e[0], f(r[2 * k + 1]) - e[1]) for k in range(3)]
        axes = [(e[2], e[3]), (-e[3], e[2])]
        for k in range(3):
            ex, ey = v[(k + 1) % 3][0] - v[k][0], v[(k + 1) % 3][1] - v[k][1]
            ln = mp.sqrt(ex * ex + ey * ey)
            if ln > 0:
                axes.append((-ey / ln, ex / ln))
        out = []
        for nx, ny in axes:
            p = [q[0] * nx + q[1] * ny for q in v]
            out.append(max(min(p) - reach(e, nx, ny), -max(p) - reach(e, nx, ny)))
        return max(out)
    a = ego(T.a[i])
    return gap(merge(a, ego(T.b[i])) if T.swept[i] else a), gap(a)


def _mpf(mp, x):
    """a longdouble as an mpf, exactly"""
    hi = np.float64(x)
    return mp.mpf(float(hi)) + mp.mpf(float(np.float64(x - hi)))


def test_double_word_gaps_agree_with_mpmath(T):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.dps = 50
    idx = np.arange(0, len(T), 5)
    assert set(T.name[idx]) == set(T.name) and set(T.oi[idx]) == set(T.oi) and set(T.hi[idx]) == set(T.hi)
    worst = 0.0
    for i in idx:
        g, gp = _mp_case(mp, T, int(i))
        worst = max(worst, float(abs(g - (_mpf(mp, T.g[i]) + _mpf(mp, T.g_lo[i])))))
        assert abs(float(gp) - float(T.g_pose[i])) <= 1e-15 * max(1.0, abs(float(gp)))
    print(f"worst |g_dd - g_mp| = {worst:.3e} m")
    assert worst <= 1e-25


# ---- the double oracle and tests/_clearance.py -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_verdicts(T):
    return C.oracle_verdicts(T)


def test_oracle_gives_the_reference_verdict_on_every_case(T, oracle_verdicts):
    pose, swept = oracle_verdicts
    bad = np.flatnonzero(swept != T.hit)
    assert not len(bad), [(T.name[i], int(T.oi[i]), int(T.hi[i]), float(T.g[i])) for i in bad[:10]]
    bad = np.flatnonzero(pose != T.hit_pose)
    assert not len(bad), [(T.name[i], int(T.oi[i]), int(T.hi[i]), float(T.g_pose[i])) for i in bad[:10]]


def test_clearance_reference_agrees_within_the_band(T):
    import _clearance as CL
    ego = CL.rect_polygon(T.a[:, 0] + C.WB * np.cos(T.a[:, 2]), T.a[:, 1] + C.WB * np.sin(T.a[:, 2]), T.a[:, 2], C.HL, C.HW)
    d = np.full(len(T), np.nan)
    m = np.flatnonzero(T.kind == "rect")
    d[m] = CL.polygon_distance(ego[m], CL.rect_polygon(*(T.row[m, q] for q in range(5))))
    m = np.flatnonzero(T.kind == "tri")
    d[m] = CL.polygon_distance(ego[m], T.row[m, :6].reshape(-1, 3, 2))
    for i in np.flatnonzero(T.kind == "circ"):
        d[i] = CL.circle_distance(ego[i:i + 1], *T.row[i, :3])[0]
    assert np.array_equal(d > 0, ~T.hit_pose)
    err = np.abs(d - np.asarray(T.dist, float))
    print(f"worst |d - exact| / B = {(err / T.B_pose).max():.3f}")
    assert np.all(err <= T.B_pose)


def test_accuracy_file_is_of_this_table(T):
    text = open(os.path.join(REPO, "profiles", "accuracy_contact.txt")).read()
    assert text.startswith(f"{len(T)} cases, B = 8 u scale")
    assert "no family exceeds it, B stays 8 u scale" in text


# ---- planted defects -------------------------------------------------------------------------------------------------------------
def _predicate(T, defect=None):
    """The pose verdict in plain doubles (NumPy), optionally with one planted defect."""
    th = T.a[:, 2]
    ux, uy = np.cos(th), np.sin(th)
    ecx, ecy = T.a[:, 0] + C.WB * ux, T.a[:, 1] + C.WB * uy
    beyond = (lambda a, b: a >= b) if defect == "open" else (lambda a, b: a > b)
    hit = np.zeros(len(T), bool)
    r = T.row
    # rectangles
    m = T.kind == "rect"
    bx, by = np.cos(r[:, 2]), np.sin(r[:, 2])
    tx, ty = r[:, 0] - ecx, r[:, 1] - ecy
    sep = np.zeros(len(T), bool)
    axes = [(ux, uy), (-uy, ux)] + ([] if defect == "no_obstacle_axes" else [(bx, by), (-by, bx)])
    for nx, ny in axes:
        re = C.HL * np.abs(ux * nx + uy * ny) + C.HW * np.abs(ux * ny - uy * nx)
        ro = r[:, 3] * np.abs(bx * nx + by * ny) + r[:, 4] * np.abs(bx * ny - by * nx)
        sep |= beyond(np.abs(tx * nx + ty * ny), re + ro)
    rb = np.hypot(r[:, 3], r[:, 4])
    d2 = tx * tx + ty * ty
    if defect == "circle_margin_0.999999":
        sep |= ~(d2 <= (C.EGO_R + rb) ** 2 * 0.999999)
    if defect == "radius_down_through_float32":
        f32 = np.float32(C.EGO_R)
        ego_r = float(f32) if float(f32) <= C.EGO_R else float(np.nextafter(f32, np.float32(0)))
        sep |= ~(d2 <= (ego_r + rb) ** 2)
    if defect == "slab_without_margin_ego_r_from_hl":
        sep |= (np.abs(tx * bx + ty * by) > r[:, 3] + C.HL) | (np.abs(ty * bx - tx * by) > r[:, 4] + C.HL)
    hit[m] = ~sep[m]
    # circles
    m = T.kind == "circ"
    lx, ly = tx * ux + ty * uy, ty * ux - tx * uy
    dx, dy = np.maximum(np.abs(lx) - C.HL, 0.0), np.maximum(np.abs(ly) - C.HW, 0.0)
    inside = (dx * dx + dy * dy < r[:, 2] ** 2) if defect == "open" else (dx * dx + dy * dy <= r[:, 2] ** 2)
    hit[m] = inside[m]
    # triangles
    for i in np.flatnonzero(T.kind == "tri"):
        v = r[i, :6].reshape(3, 2) - (ecx[i], ecy[i])
        loc = np.stack((v[:, 0] * ux[i] + v[:, 1] * uy[i], v[:, 1] * ux[i] - v[:, 0] * uy[i]), 1)
        s = False
        for nx, ny in [(1.0, 0.0), (0.0, 1.0)] + [(-(loc[(k + 1) % 3, 1] - loc[k, 1]), loc[(k + 1) % 3, 0] - loc[k, 0]) for k in range(3)]:
            p = loc[:, 0] * nx + loc[:, 1] * ny
            rr = C.HL * abs(nx) + C.HW * abs(ny)
            s |= bool(beyond(p.min(), rr) or beyond(-rr, p.max()))
        hit[i] = not s
    return hit


def test_the_plain_double_predicate_is_right_on_the_table(T):
    assert np.array_equal(_predicate(T), T.hit_pose)


@pytest.mark.parametrize("defect, family", [
    ("open", "h"),
    ("no_obstacle_axes", "d"),
    ("circle_margin_0.999999", "c"),
    ("radius_down_through_float32", "c"),
    ("slab_without_margin_ego_r_from_hl", "f"),
])
def test_planted_defect_turns_its_family_red(T, defect, family):
    wrong = _predicate(T, defect) != T.hit_pose
    red = {f: int((wrong & (T.family == f)).sum()) for f in C.FAMILIES}
    print(defect, red)
    assert red[family] >= len(C.ORIGINS) * 3, (defect, red)
    # ... at every origin, and never by calling a free pair a hit where the defect only rejects.  (The radius loses 1.6e-7 m on its
    # way through float32; at the outermost origin the smallest displacement, 64 B = 2.9e-7 m, is already larger.)
    origins = range(len(C.ORIGINS) - 1) if defect == "radius_down_through_float32" else range(len(C.ORIGINS))
    assert set(int(o) for o in T.oi[wrong & (T.family == family)]) == set(origins)
    if defect != "no_obstacle_axes":
        assert np.all(T.hit_pose[wrong])


# ---- the packing: what the GPU tests launch, through the double oracle -------------------------------------------------------------
def _oracle_batch(T, b, swept=True):
    from oracle import oracle
    s = np.arange(0.0, 8.0, 1.0)
    tb = oracle.OracleTables(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0, b.obstacles)
    K, n = b.x.shape
    p = C.params(n=n)
    hits, first_seg = np.zeros((K, n), bool), np.full(K, -1)
    for k in range(K):
        L = int(b.lengths[k])
        hits[k, :L] = oracle.check_poses(p, tb, b.x[k, :L], b.y[k, :L], b.th[k, :L])[0]
        if swept:
            first_seg[k] = oracle.check_swept(p, tb, b.x[k, :L], b.y[k, :L], b.th[k, :L])[0]
    return hits, first_seg


def test_packed_batches_give_the_reference_verdicts_through_the_oracle(T):
    batches = [(C.single_batch(T, 130), True)] + [(C.dynamic_batch(T, o), True) for o in range(len(C.ORIGINS))]
    batches += [(C.case_batch(T, o), True) for o in (0, len(C.ORIGINS) - 1)]
    for scene in range(T.n_static_scenes):
        poses, swept = C.static_batches(T, scene, pad_static=scene % 2)
        batches += [(poses, False), (swept, True)]
    seen = set()
    for b, swept in batches:
        hits, first_seg = _oracle_batch(T, b, swept)
        ph, fp, fs = b.expected(T)
        assert np.array_equal(hits, ph)
        assert not swept or np.array_equal(first_seg, fs)
        seen |= set(b.case[b.case >= 0])
    assert seen == set(range(len(T)))


def test_member_batches_hold_every_dynamic_slot_once(T):
    for o in range(len(C.ORIGINS)):
        b = C.member_batch(T, o)
        idx = T.select(static=False, scene=o)
        assert set(b.case[b.case >= 0]) == set(idx) and ((b.case >= 0).sum(axis=2) == 1).all()
        at, where = b.case.max(axis=2), b.case.argmax(axis=2)
        assert np.array_equal(where[0], where[1]) and np.array_equal(b.lengths, where[0] + 2)
        assert np.all(T.sign[at[0]] >= 0) and np.all(T.sign[at[1]] <= 0) and np.all(T.slot[at[0]] == T.slot[at[1]])
        for m in range(2):                    # the member's rows ARE the cases' rows, at the time index of the slot's first pose
            k = np.arange(len(at[m]))
            assert np.array_equal(b.members[m, k, where[m]], T.row[at[m], :5])
            assert np.isnan(b.members[m, :, :, 0]).sum() == b.members[m, :, :, 0].size - len(k)
        assert np.array_equal(b.x[k, where[0]], T.a[at[0], 0]) and np.array_equal(b.th[k, where[0] + 1], T.b[at[0], 2])


# ---- planner labels: the scenes of tests/test_contact.py against the double oracle -------------------------------------------------
@pytest.mark.parametrize("name", list(C.PLANNER_CASES))
def test_planner_scenes_are_decided_and_the_oracle_agrees(name):
    import _xref as X
    from oracle import oracle
    lo, hi, scenes = C.planner_scenes(name)
    c = X.case(name)
    inp = X.with_flags(c.inp, clear=X.FLAG_SKIP_COLLISION | X.FLAG_DRAW_ALL | X.FLAG_MATERIALIZE_ALL)
    assert len(scenes) == len(C.PLANNER_FORMS) * len(C.PLANNER_GAPS)
    lateral = np.arange(hi - lo) % len(c.inp.D)
    targeted = {s.target[0] for s in scenes}
    feasible = scenes[0].label != 0
    assert lateral[feasible].min() in lateral[list(targeted)] and lateral[feasible].max() in lateral[list(targeted)]
    for s in scenes:
        k, i = s.target
        # the targeted candidate is decided, by the gap it was given or by a deeper one of another step; it collides when that gap says so
        assert s.decided[k] and (s.gap > 0 or s.label[k] == 3), (s.form, s.gap)
        assert abs(s.gmin[k]) <= abs(s.gap) * 1.001 or s.gmin[k] < 0, (s.form, s.gap, s.gmin[k])
        others = feasible.copy()
        others[k] = False
        assert (others & ~s.decided).sum() * 8 <= others.sum(), (s.form, s.gap)
        tb = oracle.OracleTables.from_coordinate_system(c.co, s.tables)
        run = oracle.plan(inp, tb, lo, hi, want_states=False)
        lab = run.status & 3
        assert np.array_equal(lab[s.decided], s.label[s.decided]), (s.form, s.variant, s.gap)
        assert np.array_equal(lab[~feasible], (X.oracle_run(name)[0][lo:hi] & 3)[~feasible])
    # the gaps do their work: with +gap the targeted candidate is free unless another step of it is deeper in, and both labels occur
    assert {int(s.label[s.target[0]]) for s in scenes} == {1, 3}


def test_exactly_touching_cases_are_exact_and_the_oracle_calls_them_hits():
    from commonroad_rp_amd.collision import ObstacleTables
    from oracle import oracle
    ex, ey, rows = C.exact_cases()
    s = np.arange(0.0, 8.0, 1.0)
    for k in range(len(ex)):
        tb = oracle.OracleTables(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0, ObstacleTables(static_obb=rows[k:k + 1]))
        assert oracle.check_poses(C.exact_params(), tb, [ex[k]], [ey[k]], [0.0])[0][0]
        # ... and one ulp farther out along the contact normal it is free: the cases sit ON the boundary
        out = rows[k].copy()
        q = 0 if abs(out[0] - ex[k]) == C.EXACT_HL + out[3] else 1
        out[q] = np.nextafter(out[q], out[q] + (out[q] - (ex[k], ey[k])[q]))
        tb = oracle.OracleTables(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0, ObstacleTables(static_obb=out[None]))
        assert not oracle.check_poses(C.exact_params(), tb, [ex[k]], [ey[k]], [0.0])[0][0], k
