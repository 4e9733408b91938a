"""What tests/test_proj.py rests on, checked without a GPU: every case of tests/_proj.py meets the conditions of a case (the placed margin
outside 8 B with its sign, every other margin outside 1e-6 scale; nothing dropped), the double-word reference agrees with a 50-digit
evaluation of the same definition, the guard band B is at least 8 times the largest margin at which a double implementation
(oracle.frontend.project, tests/_score.project_batch, the host rp_project) decides otherwise than the reference, those three give the
reference's decision on every case, and every planted defect of the documented arithmetic turns its families red and no other."""
import numpy as np
import pytest

import _proj as P

pytestmark = pytest.mark.skipif(not P.HAVE_LONGDOUBLE, reason=P.SKIP_REASON)

BATCHES = [(name, variant) for name in P.PATHS for variant in P.variants_of(name)]
MP_UNITS = 1.0   # the double-word reference and the 50-digit evaluation agree to this many units of 2^-64 of scale


def test_paths_are_what_the_families_need():
    for name in P.PATHS:
        for variant in P.variants_of(name):
            p = P.path(name, variant)
            assert p.n_seg == (1 if name == "two" else variant) and p.n_seg <= P.LDS_ROWS + 1
            assert (np.diff(p.pos) > 0).all() and (np.abs(np.diff(p.ref, axis=0)).sum(1) > 0).all()
    ln = np.concatenate([np.diff(P.path(n, v).pos) for n, v in BATCHES])
    assert ln.min() <= 0.0100001 and abs(ln.max() - 100.0) <= 1e-6
    # the nearly straight stretch: |a| = |e . (t1 - t0)| on both sides of the switch 1e-14, going down and coming up again
    T = P.tables("straight", None)
    a = np.abs(P._f(-(T.ex * T.dtx + T.ey * T.dty)))
    below = a < 1e-14
    assert below[30:50].any() and (~below[:20]).all() and (~below[-20:]).all() and 1e-14 <= a[~below].min() < 1e-10
    origins = {tuple(np.round(P.path(n, None).ref[0], -1)) for n in P.PATHS}
    assert {(0.0, 0.0), (500.0, -500.0), (-500.0, 500.0), (3.0e6, -2.1e6)} <= origins
    assert len(P._base("serp")) - 1 == 58                       # twelve runs of three segments, eleven joints of two


@pytest.mark.parametrize("name,variant", BATCHES)
def test_every_case_meets_the_conditions_of_a_case(name, variant):
    for dl, b in P.batch(name, variant).items():
        bad = P.admission_failures(b)
        assert not bad, (dl, bad[:10])


def test_case_list_is_complete():
    rows = [r for name in P.PATHS for r in P.cases(name)]
    by = {f: [r for r in rows if r.family == f] for f in P.FAMILIES}
    for fam in ("medial", "ends"):                       # both signs at all three displacements, on every label
        for label in {r.label for r in by[fam]}:
            assert {(r.level, r.sign) for r in by[fam] if r.label == label} == {(lv[0], sg) for lv in P.LEVELS for sg in (1, -1)}, label
    placed_limit = [r for r in by["limit"] if r.kind == "limit"]
    for label in {r.label for r in placed_limit}:
        assert {(r.level, r.sign) for r in placed_limit if r.label == label} == {(lv[0], sg) for lv in P.LEVELS for sg in (1, -1)}, label
    assert {r.d_limit for r in by["limit"]} == {20.0, 2.0, 0.5} and any(r.label == "runner_at_limit" for r in by["limit"])
    assert {r.path for r in by["medial"]} == {"u", "serp"} and any(r.label == "legs_k5" for r in by["medial"])   # (k5: inside the bend)
    assert {r.label.split("_")[0] for r in by["ends"]} == {"first", "last"} and {r.variant for r in by["ends"]} == {None} | set(P.VARIANTS)
    assert {r.path for r in by["vnormal"]} >= {"arc6", "scurve"} and {0.0, 15.0, -15.0} <= {float(r.label.split("_d")[1]) for r in by["vnormal"]}
    tied = {n: [r for r in by["ties"] if r.path == n and r.level == "tied"] for n in ("u_axis", "serp", "laps")}
    assert len(tied["laps"]) >= 130 and all(tied.values())
    b = P.batch("laps", P.VARIANTS[0])[20.0]
    n_tied = {int(b.truth.n_tied[i]) for i, r in enumerate(b.rows) if r.level == "tied"}
    assert n_tied == {2, 3, 11}, n_tied
    levels = [r.level for r in b.rows]
    assert all(levels[i] != levels[i + 1] for i in range(len(levels) - 1))               # tied and untied lanes alternate
    # the focal family: draws within a sagitta of a bend's centre, beyond it, beside the caustic of the S-curve's kink and inside the U's corners
    assert {r.level for r in by["focal"]} == {"centre", "beyond", "caustic", "corner"} and {r.path for r in by["focal"]} == set(P.FOCAL_LIMIT)
    for name in P.FOCAL_LIMIT:
        admitted = sum(r.path == name for r in by["focal"])
        print(f"focal, {name}: {P.FOCAL_TRIED} drawn, {admitted} admitted")
        assert admitted >= P.FOCAL_TRIED // 2
    b = P.batch("u_axis", P.VARIANTS[0])[20.0]                                          # ... where disc takes either sign beside the window
    T = P.tables("u_axis", P.VARIANTS[0])
    corner = np.flatnonzero([r.level == "corner" for r in b.rows])
    ip, ik = P.open_pairs(T, b.x[corner], b.y[corner], 20.0)
    c = P.candidates(T, ik, b.x[corner][ip], b.y[corner][ip])
    no_root, two = ~c.lin & ~c.have[0], c.adm.sum(0) == 2
    assert len(set(ip[no_root])) >= 40 and two.any() and len(set(ip[~c.lin & c.have[0]])) == len(corner)
    print({f: len(v) for f, v in by.items()})


def _mp_point(mp, p, tan, ks, x, y, d_limit):
    """the definition of tests/_proj.py's docstring for ONE point over the segments ks, at mp's precision -> (seg, root, s, d, lam, gap)"""
    F = mp.mpf
    cands = []
    for k in ks:
        p0x, p0y, p1x, p1y = (F(float(q)) for q in (*p.ref[k], *p.ref[k + 1]))
        ex, ey, qx, qy = p1x - p0x, p1y - p0y, F(x) - p0x, F(y) - p0y
        (t0x, t0y), (t1x, t1y) = tan[k], tan[k + 1]
        dtx, dty = t1x - t0x, t1y - t0y
        a, b, c = -(ex * dtx + ey * dty), (qx * dtx + qy * dty) - (ex * t0x + ey * t0y), qx * t0x + qy * t0y
        if a == 0:
            roots = [-c / b] if b != 0 else []
        else:
            disc = b * b - 4 * a * c
            if disc < 0:
                continue
            with mp.workdps(3 * mp.mp.dps):       # (the textbook form: with |a| down to 1e-32 it cancels 35 digits of -b -+ sqrt(disc))
                sq = mp.sqrt(b * b - 4 * a * c)
                roots = [(-b + sq) / (2 * a), (-b - sq) / (2 * a)]
            roots = [+r for r in roots]
        for r, lam in enumerate(roots):
            if not (-F(P.W_LO) <= lam <= F(P.W_HI)):
                continue
            lam = min(max(lam, F(0)), F(1))
            tx, ty = t0x + lam * dtx, t0y + lam * dty
            fx, fy = p0x + lam * ex, p0y + lam * ey
            d = (-(F(x) - fx) * ty + (F(y) - fy) * tx) / mp.sqrt(tx * tx + ty * ty)
            if abs(d) <= F(d_limit):
                s = F(float(p.pos[k])) + lam * (F(float(p.pos[k + 1])) - F(float(p.pos[k])))
                cands.append((abs(d), k, r, s, d, lam))
    if not cands:
        return None
    best = min(cands, key=lambda q: q[:3])
    apart = [q[0] for q in cands if abs(q[3] - best[3]) > P.S_APART]
    return best[1], best[2], best[3], best[4], best[5], (min(apart) - best[0]) if apart else None


def _mpf(mp, v):
    """a longdouble as an mpf, exactly: its leading 53 bits and the rest"""
    head = float(v)
    return mp.mpf(head) + mp.mpf(float(v - np.longdouble(head)))


def gap_scale(T, b, t, i):
    """the scale the reference divided the gap of row i by: the winner's and the runner-up's |x| + |y| + |foot_x| + |foot_y|"""
    tot = 0.0
    for k, s in ((int(t.seg[i]), float(t.s[i])), (int(t.runner_seg[i]), float(t.runner_s[i]))):
        lam = (s - b.path.pos[k]) / (b.path.pos[k + 1] - b.path.pos[k])
        foot = b.path.ref[k] + lam * (b.path.ref[k + 1] - b.path.ref[k])
        tot += abs(b.x[i]) + abs(b.y[i]) + abs(foot[0]) + abs(foot[1])
    return tot


def test_reference_against_fifty_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    F = mp.mpf
    worst, checked, where = 0.0, 0, None
    for name in P.PATHS:
        variant = P.variants_of(name)[0]
        p, T = P.path(name, variant), P.tables(name, variant)
        u = []
        for k in range(p.n_seg):
            ex, ey = F(float(p.ref[k + 1, 0])) - F(float(p.ref[k, 0])), F(float(p.ref[k + 1, 1])) - F(float(p.ref[k, 1]))
            ln = mp.sqrt(ex * ex + ey * ey)
            u.append((ex / ln, ey / ln))
        tan = [u[0]] + [None] * (p.n_seg - 1) + [u[-1]]
        for k in range(1, p.n_seg):
            sx, sy = u[k - 1][0] + u[k][0], u[k - 1][1] + u[k][1]
            sn = mp.sqrt(sx * sx + sy * sy)
            tan[k] = (sx / sn, sy / sn)
        for dl, b in P.batch(name, variant).items():
            t = b.truth
            ip, ik = P.open_pairs(T, b.x, b.y, dl)
            for i in range(0, len(b.rows), 9):
                got = _mp_point(mp, p, tan, ik[ip == i], float(b.x[i]), float(b.y[i]), dl)
                checked += 1
                if got is None:
                    assert not t.inside[i], (name, b.rows[i].label)
                    continue
                seg, root, s, d, lam, gap = got
                if b.rows[i].family == "vnormal":     # (the twin segments hold the same clamped foot point: equal |d|, up to the 50th digit)
                    assert t.inside[i] and {seg, int(t.seg[i])} <= {b.rows[i].vertex - 1, b.rows[i].vertex}, (name, b.rows[i].label, seg)
                else:
                    assert t.inside[i] and (seg, root) == (int(t.seg[i]), int(t.root[i])), (name, b.rows[i].label, seg, root)
                scale = abs(b.x[i]) + abs(b.y[i]) + abs(float(p.ref[seg, 0])) + abs(float(p.ref[seg, 1])) + abs(float(s))
                for mine, theirs in ((t.s_dd[i], s), (t.d_dd[i], d)):
                    err = abs(_mpf(mp, mine.hi) + _mpf(mp, mine.lo) - theirs)
                    if float(err / scale) * 2.0 ** 64 > worst:
                        worst, where = float(err / scale) * 2.0 ** 64, (name, dl, b.rows[i].family, b.rows[i].label, b.rows[i].level)
                if gap is None:
                    assert t.gap[i] == np.inf
                else:
                    assert (gap == 0) == bool(t.gap_zero[i])
                    assert abs(float(gap) - float(t.gap[i]) * gap_scale(T, b, t, i)) <= 1e-14 * scale      # (the margin is kept as a float64)
    print(f"{checked} points, largest |double-word - 50 digits| = {worst:.2e} units of 2^-64 of scale at {where}")
    assert checked >= 150 and worst <= MP_UNITS


def test_guard_band_is_eight_times_what_the_double_implementations_need():
    res = P.measure()
    for kind, (draws, worst) in res.items():
        print(f"{kind}: {draws} draws, worst |margin| with another decision {worst:.3f} u scale, BAND {P.BAND[kind]}")
        assert draws >= 300 and P.BAND[kind] >= 8.0 * worst, kind
        band = P.BAND[kind]
        assert band == 2.0 ** round(np.log2(band))      # a power of two times u scale


@pytest.mark.parametrize("name,variant", BATCHES)
def test_double_implementations_decide_as_the_reference(name, variant):
    for dl, b in P.batch(name, variant).items():
        for key, (ins, s, d) in P.doubles(b.path, b.x, b.y, dl, which=("numpy", "host") if variant == P.VARIANTS[1] else ("oracle", "numpy", "host")).items():
            got = P.NS(s=s, d=d, seg=b.numpy.seg if key == "numpy" else None)
            bad = P.decision_failures(b, got)
            assert not bad, (key, dl, bad[:5])
            exact_rows = np.array([r.level in ("tied", "exact") for r in b.rows])
            if exact_rows.any():                       # every operation is exact there: the three agree bit for bit
                assert np.array_equal(s[exact_rows], b.numpy.s[exact_rows]) and np.array_equal(d[exact_rows], b.numpy.d[exact_rows]), key


def _red(defect):
    """(families with a wrong decision: their levels, families outside the value rule, paths with either)"""
    dec, val, paths = {}, set(), set()
    for name in P.PATHS:
        variant = P.variants_of(name)[0]
        for dl, b in P.batch(name, variant).items():
            got = P.restated(b.path, b.x, b.y, dl, defect)
            for q in P.decision_failures(b, got):
                dec.setdefault(q[1], set()).add(q[3])
                paths.add(name)
            lines = P.value_failures(b, got, rows=("s", "d"))
            val |= {line.split()[1] for line in lines}
            paths |= {name} if lines else set()
    return dec, val, paths


def test_restatement_without_a_defect_is_green():
    assert _red(None) == ({}, set(), set())


def test_planted_defects_turn_their_families_red():
    """le_for_lt: the LAST of equal candidates wins -- the exact ties, and the rows exactly at the limit, which are tied too.
    lt_at_limit: |d| == d_limit exactly is outside -- only the exact rows of the limit family have that.
    window_0: roots in [-1e-12, 0) and (1, 1 + 1e-12] are lost -- the ends family (on a vertex normal the twin segment still holds the point:
              the decision stays, the values move).
    textbook_root: the paths with segments of 1e-14 <= |a| < 1e-10 -- the nearly straight stretch, the rotated U's legs, the arc at the
              origin 3e6 (vertices rounded to 5e-10 m) and the S-curve's 0.01 m segments -- and every family with cases on those segments;
              never the ends (their roots sit on the first and last segment, |a| < 1e-14 or > 1e-10), the ties or the list edge (a = 0).
    second_root_dropped: with b < 0, the usual sign, the admissible root is the second one -- every family with a curved segment.
    disc_gt_0: differs only where b * b - 4.0 * a * c == 0.0 in doubles.  No case of the families has that (their margins keep 8 B); the
              rows of ``disc_zero_cases`` do: the double root is their only candidate, and `>` loses it."""
    dec, val, _ = _red("le_for_lt")
    assert dec == {"ties": {"tied"}, "limit": {"exact"}} and not val
    dec, val, _ = _red("lt_at_limit")
    assert dec == {"limit": {"exact"}} and not val
    dec, val, _ = _red("window_0")
    assert set(dec) == {"ends"} and val <= {"vnormal"}
    dec, val, paths = _red("textbook_root")
    small = set()
    for name in P.PATHS:
        T = P.tables(name, None)
        a = np.abs(P._f(-(T.ex * T.dtx + T.ey * T.dty)))
        if ((a >= 1e-14) & (a < 1e-10)).any():
            small.add(name)
    assert small == {"u", "arc6", "scurve", "straight"} and paths == small
    assert set(dec) | val == {"medial", "vnormal", "limit", "straight", "focal"} and {"straight", "limit", "vnormal", "focal"} <= val
    dec, val, _ = _red("second_root_dropped")
    assert set(dec) == {"vnormal", "medial", "focal", "ends", "limit", "straight"}          # (all but the ties and the list edge: a = 0 there)
    assert _red("disc_gt_0") == ({}, set(), set())
    p, x, y = P.disc_zero_cases()
    assert len(x) >= 20
    for defect in (None,) + tuple(q for q in P.DEFECTS if q != "disc_gt_0"):
        got = P.restated(p, x, y, 20.0, defect)
        assert (got.seg == 0).all() and (got.lam > 0.15).all() and (got.lam < 0.85).all(), defect
    assert (P.restated(p, x, y, 20.0, "disc_gt_0").seg == -1).all()


@pytest.mark.parametrize("name", P.LIFT_PATHS)
def test_lift_and_back_cases(name):
    """s on every vertex and one double on either side: the header's rule puts pos[k] on segment k (the last vertex: on the last segment),
    the double below it on k - 1, the doubles outside the two ends off the path; nearly every preimage is unique; the oracle's own lift
    and way back pass what the device is held to, and a lift that puts s == pos[k] on segment k - 1 does not."""
    for variant in P.VARIANTS:
        lb = P.lift_batch(name, variant)
        n = len(lb.path.pos)
        seg = lb.truth.seg.reshape(n, 3)
        k = np.arange(n)
        assert seg[0, 0] == -1 and seg[-1, 2] == -1 and int((~lb.truth.on).sum()) == 2
        assert np.array_equal(seg[1:, 0], k[1:] - 1) and np.array_equal(seg[:, 1], np.minimum(k, n - 2)) and np.array_equal(seg[:-1, 2], k[:-1])
        assert np.array_equal(lb.oracle.seg, lb.truth.seg)
        assert lb.unique.sum() >= 0.99 * lb.truth.on.sum() and set(np.abs(lb.d[lb.unique])) == set(np.abs(P.LIFT_D))
        n_off = int((~lb.truth.on).sum())
        assert not P.lift_failures(lb, lb.oracle.x, lb.oracle.y, lb.oracle.seg, n_off, lb.oracle.s, lb.oracle.d)
        wrong = np.where(lb.truth.on & (np.arange(lb.s.size) % 3 == 1) & (lb.truth.seg > 0), lb.truth.seg - 1, lb.truth.seg)
        assert P.lift_failures(lb, lb.oracle.x, lb.oracle.y, wrong, n_off, lb.oracle.s, lb.oracle.d)
        far = P.NS(**vars(lb.oracle))
        assert P.lift_failures(lb, far.x + 1e-9, far.y, far.seg, n_off, None, None)                  # a position 1e-9 m off is seen
