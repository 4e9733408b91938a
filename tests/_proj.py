"""The curvilinear projection at its edges, against an exact reference (TEST INFRASTRUCTURE: tests/test_proj_abi.py on the CPU,
tests/test_proj.py on the GPU).

TRUTH: the projection of csrc/rp_frontend.h / include/rp_score.h as the real-number function of its DOUBLE inputs (vertices, ref_pos,
ref_theta, the point, d_limit), evaluated in the double-word longdouble arithmetic of tests/_dd.py:
  vertex tangents   the exactly normalised sums of the adjacent unit directions (the two end vertices: the end segment's direction);
  per segment       the real roots of c + b lam + a lam^2 = 0,  a = -(e . dt),  b = q . dt - e . t0,  c = q . t0,  q = P - p0, in the order
                    (-b + sqrt(disc)) / 2a, (-b - sqrt(disc)) / 2a (a = 0: the one root -c / b); a root is admissible inside
                    [-1e-12, 1 + 1e-12] (the doubles 1e-12 and 1.0 + 1e-12) and is then clamped to [0, 1];
  per root          d = cross(t(lam) / |t(lam)|, P - foot),  s = pos0 + lam (pos1 - pos0),  theta_ref = theta0 + lam (theta1 - theta0);
  the winner        the smallest |d| <= d_limit; ties go to the first segment, then to the first root.
The switch |a| < 1e-14 of the double code is no part of the truth: below it the second root lies 1e14 segments away.

MARGINS, each divided by its SCALE (the magnitudes of the terms it is formed from, summed), so that 1.0 u = 2^-53 is one rounding:
  gap      |d| of the runner-up (an eligible candidate whose s is more than 1e-6 m from the winner's) - |d| of the winner; scale = the two
           candidates' |x| + |y| + |foot_x| + |foot_y|
  limit    d_limit - |d| of every admissible root; the one nearest to 0; scale = d_limit + the candidate's scale as above
  window   lam + 1e-12 and 1 + 1e-12 - lam of every root that could change the result (|d| within 1e-3 m of the winner's, or of d_limit
           where nothing wins); scale = 1 + (|q_x t0_x| + |q_y t0_y|) / |b|
  disc     b^2 - 4 a c of every such segment whose root pair lies within half a segment of the window; scale = b^2 + 4 |a c|

GUARD BAND  B[kind] = BAND[kind] u scale.  Nothing from the device enters it: ``measure`` draws double points beside each edge, asks
oracle.frontend.project, tests/_score.project_batch and the host rp_project, and records the largest |margin| at which one of them
decides otherwise than the truth; tests/test_proj_abi.py asserts BAND >= 8 times that.

A CASE is one point with ONE margin placed beside its edge: the edge is found by bisection on the truth's margin along a direction that
moves it, the point displaced to +-64 B, +-2^16 B and +-1e-6 scale, rounded to doubles and re-evaluated: the placed margin keeps its sign
with |g| >= 8 B, every other margin of the point is >= 1e-6 scale -- conditions on the generator, asserted, never a reason to drop a case
(``admission_failures``).  Families: medial limit ends vnormal straight focal ties.  ``focal`` alone selects: of the points drawn inside a
bend beyond its centre those are cases whose winner leads by >= 8 B (the table says how many).  ``vnormal`` (points on the normal through an interior
vertex, where segments k - 1 and k hold the same foot point) and ``straight`` (values only) place no margin; what they need is that no
rounding decides anything else at the point, and the placed families show that 64 B is enough for that: their other margins are held
to 2^16 B (1e-6 scale is 12 m at the origin (3e6, -2.1e6), twice the radius of the arc that lies there).  ``ties`` are built so that
every double operation is exact and the gap is 0 in both words.

LIFT AND BACK (``lift_exact``, ``lift_batch``): include/rp_lift.h's point rule in the same arithmetic, for (s, d) on and beside every vertex.
``disc_zero_cases``: rows of the documented double arithmetic where disc == 0.0, for the NumPy restatement alone.

usage: python tests/_proj.py [out_file]      writes profiles/accuracy_projection.txt (on a GPU box: with the device's distances)"""
import functools
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

if __name__ == "__main__":   # (as a script: the paths tests/conftest.py sets up for the suite)
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "commonroad-reactive-planner_amd"), os.path.join(_repo, "tests")]

import _dd as dd
from _dd import DD
from _xref import HAVE_LONGDOUBLE, SKIP_REASON, MARGIN_MAX, MARGIN_RMS, FLOOR_MAX, FLOOR_RMS   # noqa: F401
import _score as S

from oracle import frontend

LD = np.longdouble
U = 2.0 ** -53
KINDS = ("gap", "limit", "window")
BAND = {"gap": 64.0, "limit": 64.0, "window": 64.0}     # B = BAND u scale (see ``measure`` for what stands behind it)
DECIDED = 8.0                                            # the placed margin: |g| >= DECIDED B
OTHER = 1e-6                                             # every other margin: |g| >= OTHER scale
OTHER_UNPLACED = 65536.0                                 # ... of the families that place none: this many B (see the docstring)
LEVELS = (("64B", 64.0, None), ("65536B", 65536.0, None), ("1e-6", None, 1e-6))
FAMILIES = ("medial", "limit", "ends", "vnormal", "straight", "focal", "ties", "listedge")
FOCAL_TRIED = 160                                        # candidates drawn per bend; admitted: those whose winner leads by >= 8 B
FOCAL_LIMIT = {"arc6": 20.0, "arc25": 80.0, "scurve": 20.0, "u_axis": 20.0}
W_LO, W_HI = 1e-12, 1.0 + 1e-12
S_APART = 1e-6                                           # a runner-up is a candidate whose s differs by more than this
LDS_ROWS = S.LDS_ROWS
VARIANTS = (LDS_ROWS, LDS_ROWS + 1)
SC_LIST = 8


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _f(a):
    """a double-word or longdouble array rounded to float64 (for scales and reports, never for a decision)"""
    return np.asarray(a.ld() if isinstance(a, DD) else a).astype(np.float64)


def to_double(a):
    """a double-word array CORRECTLY rounded to float64 (one rounding, not two)"""
    x = _f(a)
    best, err = x.copy(), _f(abs(a - DD(_ld(x))))
    for nb in (np.nextafter(x, -np.inf), np.nextafter(x, np.inf)):
        e = _f(abs(a - DD(_ld(nb))))
        take = e < err
        best, err = np.where(take, nb, best), np.where(take, e, err)
    return best


# ---- the paths -----------------------------------------------------------------------------------------------------------------
def _rot(pts, angle, origin):
    c, s = math.cos(angle), math.sin(angle)
    return np.asarray(pts, float) @ np.array([[c, s], [-s, c]]) + np.asarray(origin, float)


def _from_headings(lengths, headings, start=(0.0, 0.0)):
    step = np.stack((lengths * np.cos(headings), lengths * np.sin(headings)), 1)
    return np.concatenate(([start], np.asarray(start) + np.cumsum(step, axis=0)))


def _arc(radius, sweep, seg):
    n = int(round(radius * sweep / seg))
    ang = np.linspace(0.0, sweep, n + 1)
    return np.stack((radius * np.sin(ang), radius * (1.0 - np.cos(ang))), 1)


def _runs(plan):
    """Axis-parallel runs of 8 m segments at dyadic coordinates, joined by two diagonal segments: plan = [(y, x_from, x_to), ...]"""
    pts = []
    for j, (y, x0, x1) in enumerate(plan):
        xs = np.arange(x0, x1 + (8 if x1 > x0 else -8), 8.0 if x1 > x0 else -8.0)
        pts += [(float(x), float(y)) for x in xs]
        if j + 1 < len(plan):
            yn = plan[j + 1][0]
            half = 0.5 * abs(yn - y)
            pts.append((x1 + (half if x1 > x0 else -half), 0.5 * (y + yn)))
    return np.array(pts)


def _base(name):
    if name == "u":          # legs 3.5 m apart, rotated and translated
        bend = 1.75 * np.stack((np.sin(np.linspace(0, np.pi, 7)), 1.0 - np.cos(np.linspace(0, np.pi, 7))), 1)[1:-1]
        leg = np.arange(0.0, 30.1, 5.0)
        pts = np.concatenate((np.stack((leg, 0 * leg), 1), bend + [30.0, 0.0], np.stack((leg[::-1], 0 * leg + 3.5), 1)))
        return _rot(pts, 0.3, (500.0, -500.0))
    if name == "u_axis":     # the U of tests/_score.py: dyadic, axis-parallel
        return S.U_PATH.copy()
    if name == "serp":       # twelve parallel runs 4 m apart
        return _runs([(4.0 * j, 0.0, 24.0) if j % 2 == 0 else (4.0 * j, 24.0, 0.0) for j in range(12)]) + [-500.0, 500.0]
    if name == "laps":       # runs that lie ON each other: 2 tied runs for x in (48, 56), 3 in (24, 40), 11 in (8, 16), all at y = 2
        plan = [(0.0, 0.0, 64.0), (4.0, 64.0, 0.0), (0.0, 0.0, 48.0), (8.0, 48.0, 0.0)]
        plan += [(0.0, 0.0, 24.0) if j % 2 == 0 else (4.0, 24.0, 0.0) for j in range(8)]
        return _runs(plan)
    if name == "stack":      # nine forward runs almost ON each other, each 2^-10 m nearer to the points below them than the one before
        plan = []
        for j in range(9):
            plan += [(-j / 1024.0, 0.0, 24.0), (8.0, 24.0, 0.0)]
        return _runs(plan[:-1])
    if name == "arc6":
        return _rot(_arc(6.0, 1.5 * np.pi, 0.25), 0.7, (3.0e6, -2.1e6))
    if name == "arc25":
        return _rot(_arc(25.0, 2.0, 0.5), -0.4, (0.0, 0.0))
    if name == "scurve":     # an S of 0.5 m segments with twenty 0.01 m segments in it
        ln = np.concatenate((np.full(60, 0.5), np.full(20, 0.01), np.full(60, 0.5)))
        sarc = np.concatenate(([0.0], np.cumsum(ln)))[:-1]
        return _from_headings(ln, 0.9 * np.sin(sarc / 10.0) + 0.2, (-500.0, 500.0))
    if name == "two":
        return np.array([[3.0, -2.0], [83.0, 38.0]])
    if name == "straight":   # heading change per segment from 1e-2 down to 1e-10 rad and up again: |a| crosses 1e-14 both ways
        j = np.arange(41)
        delta = 1e-2 * 10.0 ** (-8.0 * j / 40.0)
        delta = np.concatenate((delta, delta[::-1][1:]))
        return _from_headings(np.full(len(delta), 1.0), 0.5 + np.cumsum(delta))
    raise KeyError(name)


PATHS = ("u", "u_axis", "serp", "laps", "stack", "arc6", "arc25", "scurve", "two", "straight")
TAIL = (100.0, 40.0, 10.0)   # the tail that fills a table up to its row count: straight on from the last vertex


@functools.lru_cache(maxsize=None)
def path(name, n_seg=None):
    """A path as a namespace (ref, pos, theta), filled up to n_seg segments by a straight tail (None, and ``two``: as it is)."""
    pts = _base(name)
    if n_seg is not None and name != "two":
        extra = n_seg - (len(pts) - 1)
        assert extra >= 2, (name, extra)
        e = pts[-1] - pts[-2]
        e = e / math.hypot(*e)
        if name in ("u_axis", "serp", "laps", "stack"):
            e = np.round(e)
        run = np.cumsum(np.resize(TAIL, extra))
        pts = np.concatenate((pts, pts[-1] + run[:, None] * e))
    pos = frontend.compute_pathlength_from_polyline(pts)
    theta = np.unwrap(frontend.compute_orientation_from_polyline(pts))
    for q in (pts, pos, theta):
        q.setflags(write=False)
    return NS(name=name, ref=pts, pos=pos, theta=theta, n_seg=len(pts) - 1)


@functools.lru_cache(maxsize=None)
def tables(name, n_seg=None):
    """the per-segment quantities of the truth, double-word arrays [n_seg]"""
    p = path(name, n_seg)
    X, Y = DD(_ld(p.ref[:, 0])), DD(_ld(p.ref[:, 1]))
    ex, ey = X[1:] - X[:-1], Y[1:] - Y[:-1]
    ln = dd.sqrt(ex * ex + ey * ey)
    ux, uy = ex / ln, ey / ln
    n = len(p.pos)
    tx, ty = dd.zeros(n), dd.zeros(n)
    tx[0], ty[0], tx[n - 1], ty[n - 1] = ux[0], uy[0], ux[n - 2], uy[n - 2]
    if n > 2:
        sx, sy = ux[:-1] + ux[1:], uy[:-1] + uy[1:]
        sn = dd.sqrt(sx * sx + sy * sy)
        tx[1:n - 1], ty[1:n - 1] = sx / sn, sy / sn
    P, Th = DD(_ld(p.pos)), DD(_ld(p.theta))
    ctr = p.ref[:-1] + 0.5 * np.diff(p.ref, axis=0)
    rad = 0.5 * np.sqrt((np.diff(p.ref, axis=0) ** 2).sum(1)) * (1.0 + 1e-12)
    return NS(path=p, px=X[:-1], py=Y[:-1], ex=ex, ey=ey, t0x=tx[:-1], t0y=ty[:-1], dtx=tx[1:] - tx[:-1], dty=ty[1:] - ty[:-1],
              pos0=P[:-1], dpos=P[1:] - P[:-1], th0=Th[:-1], dth=Th[1:] - Th[:-1], ctr=ctr, rad=rad, n_seg=n - 1)


# ---- the truth -------------------------------------------------------------------------------------------------------------------
def _iszero(a):
    return (a.hi == 0) & (a.lo == 0)


def candidates(T, k, x, y):
    """Both roots of segments k [M] for points x, y [M] (doubles): arrays [2, M].  have: the root exists; adm: inside the window;
    ad, d, s, lam (clamped), th: double-word; wlo, whi: signed distances to the window's edges; disc; and the scales."""
    k = np.asarray(k)
    Xp, Yp = DD(_ld(x)), DD(_ld(y))
    g = lambda q: q[k]   # noqa: E731
    px, py, ex, ey, t0x, t0y, dtx, dty = (g(q) for q in (T.px, T.py, T.ex, T.ey, T.t0x, T.t0y, T.dtx, T.dty))
    qx, qy = Xp - px, Yp - py
    a = -(ex * dtx + ey * dty)
    b = (qx * dtx + qy * dty) - (ex * t0x + ey * t0y)
    c = qx * t0x + qy * t0y
    lin = _iszero(a)
    disc = b * b - (a * c).scaled(4.0)
    real = np.asarray(disc >= 0)
    one = DD(np.ones(k.shape, dtype=LD))
    sq = dd.sqrt(dd.where(real, disc, dd.zeros(k.shape)))
    bpos = np.asarray(b >= 0)
    q = -dd.where(bpos, b + sq, b - sq).scaled(0.5)
    qzero = _iszero(q)
    cq, qa = c / dd.where(qzero, one, q), q / dd.where(lin, one, a)
    bzero = _iszero(b)
    r_lin = -(c / dd.where(bzero, one, b))
    zero = dd.zeros(k.shape)
    r0 = dd.where(lin, r_lin, dd.where(qzero, zero, dd.where(bpos, cq, qa)))
    r1 = dd.where(qzero, zero, dd.where(bpos, qa, cq))
    have = np.stack((np.where(lin, ~bzero, real), ~lin & real))
    lam = dd.stack((r0, r1))
    wlo, whi = lam + DD(LD(W_LO)), DD(LD(W_HI)) - lam
    adm = have & np.asarray(wlo >= 0) & np.asarray(whi >= 0)
    lamc = dd.where(np.asarray(lam < 0), dd.zeros(lam.shape), dd.where(np.asarray(lam > 1), DD(np.ones(lam.shape, dtype=LD)), lam))
    lamc = dd.where(have, lamc, dd.zeros(lam.shape))
    tx, ty = t0x + lamc * dtx, t0y + lamc * dty
    tn = dd.sqrt(tx * tx + ty * ty)
    fx, fy = px + lamc * ex, py + lamc * ey
    d = (-((Xp - fx) * ty) + (Yp - fy) * tx) / tn
    s = g(T.pos0) + lamc * g(T.dpos)
    th = g(T.th0) + lamc * g(T.dth)
    sc_d = np.abs(x) + np.abs(y) + np.abs(_f(fx)) + np.abs(_f(fy))
    with np.errstate(all="ignore"):
        sc_w = 1.0 + (np.abs(_f(qx * t0x)) + np.abs(_f(qy * t0y))) / np.abs(_f(b))
    sc_disc = _f(b * b) + 4.0 * np.abs(_f(a * c))
    mid = _f(-(b / dd.where(lin, one, a)).scaled(0.5))   # -b / 2a: where the root pair meets
    return NS(have=have, adm=adm, lam=lamc, raw=lam, ad=abs(d), d=d, s=s, th=th, wlo=wlo, whi=whi, disc=disc, lin=lin, mid=mid,
              sc_d=np.broadcast_to(sc_d, lam.shape), sc_w=np.broadcast_to(sc_w, lam.shape), sc_disc=sc_disc)


def open_pairs(T, x, y, reach):
    """(point, segment) pairs that can hold a candidate within ``reach``: |d| is the distance to the foot point, the foot point lies
    in the segment's circle.  1e-3 m of slack: a thousand million times what the clamping of lam by 1e-12 segments moves a foot point."""
    dist = np.hypot(T.ctr[None, :, 0] - x[:, None], T.ctr[None, :, 1] - y[:, None])
    return np.nonzero(dist - T.rad[None] <= reach + 1e-3)


def _first(p, n, keys):
    """Per point 0 .. n - 1 the index of the lexicographically smallest row of ``keys`` (most significant first); -1: none"""
    out = np.full(n, -1)
    if p.size:
        order = np.lexsort(tuple(reversed((p,) + tuple(keys))))   # (lexsort: the LAST key is the primary one)
        ps = p[order]
        first = np.concatenate(([True], ps[1:] != ps[:-1]))
        out[ps[first]] = order[first]
    return out


def exact(name, n_seg, x, y, d_limit, theta=None):
    """The truth for points x, y [P]: seg, root, inside; s, d, lam, theta_cl (double-word, rounded to longdouble; NaN outside); the
    margins over their scales gap, limit, window, disc (float64, inf: no such decision at this point) and n_tied (eligible candidates at
    the winner's |d| in both words, itself included)."""
    T = tables(name, n_seg)
    x, y = np.asarray(x, float).ravel(), np.asarray(y, float).ravel()
    P = x.size
    ip, ik = open_pairs(T, x, y, d_limit)
    c = candidates(T, ik, x[ip], y[ip])
    M = ip.size
    pp, kk, rr = np.concatenate((ip, ip)), np.concatenate((ik, ik)), np.repeat([0, 1], M)
    flat = lambda q: DD(q.hi.reshape(-1), q.lo.reshape(-1)) if isinstance(q, DD) else np.asarray(q).reshape(-1)   # noqa: E731
    adm, ad, s, d, lam, th = flat(c.adm), flat(c.ad), flat(c.s), flat(c.d), flat(c.lam), flat(c.th)
    lim = DD(LD(d_limit)) - ad
    elig = adm & np.asarray(lim >= 0)
    idx = np.flatnonzero(elig)
    w = _first(pp[idx], P, (ad.hi[idx], ad.lo[idx], kk[idx], rr[idx]))
    inside = w >= 0
    win = np.where(inside, idx[np.maximum(w, 0)] if idx.size else 0, 0)
    pick = lambda q: dd.where(inside, q[win], DD(np.full(P, np.nan, dtype=LD)))   # noqa: E731
    out = NS(seg=np.where(inside, kk[win], -1), root=np.where(inside, rr[win], -1), inside=inside, s=pick(s).ld(), d=pick(d).ld(), lam=pick(lam).ld(),
             s_dd=pick(s), d_dd=pick(d))
    if theta is not None:
        two_pi = dd.PIO2.scaled(4.0)
        m = dd.mod(DD(_ld(theta)) - dd.where(inside, th[win], dd.zeros(P)), two_pi)
        m = dd.where(np.asarray(m >= dd.PIO2.scaled(2.0)), m - two_pi, m)
        out.theta_cl = np.where(inside, m.ld(), LD(np.nan))
    # ---- margins ----
    ad_w, s_w = ad[win], s[win]
    sc_d = flat(c.sc_d)
    # gap: eligible candidates whose s differs
    apart = elig & inside[pp] & (np.abs(_f(s - s_w[pp])) > S_APART)
    ia = np.flatnonzero(apart)
    ru = _first(pp[ia], P, (ad.hi[ia], ad.lo[ia]))
    has_ru = ru >= 0
    rwin = np.where(has_ru, ia[np.maximum(ru, 0)] if ia.size else 0, 0)
    gap = ad[rwin] - ad_w
    out.gap = np.where(has_ru, _f(gap) / (sc_d[win] + sc_d[rwin]), np.inf)
    out.gap_zero = has_ru & _iszero(gap)
    out.runner_seg = np.where(has_ru, kk[rwin], -1)
    out.runner_s = np.where(has_ru, _f(s[rwin]), np.nan)
    tied = elig & inside[pp] & _iszero(ad - ad_w[pp])
    out.n_tied = np.bincount(pp[tied], minlength=P)
    # limit: every admissible root
    q = np.where(adm, np.abs(_f(lim)) / (d_limit + sc_d), np.inf)
    out.limit = np.full(P, np.inf)
    np.minimum.at(out.limit, pp, q)
    out.limit_signed = np.where(inside, _f(DD(LD(d_limit)) - ad_w) / (d_limit + sc_d[win]), np.nan)
    # window and disc: roots that could change the result
    reach = np.where(inside, _f(ad_w), d_limit)[pp] + 1e-3
    matters = flat(c.have) & (_f(ad) <= reach)
    wmin = np.minimum(np.abs(_f(flat(c.wlo))), np.abs(_f(flat(c.whi)))) / flat(c.sc_w)
    out.window = np.full(P, np.inf)
    np.minimum.at(out.window, pp, np.where(matters, wmin, np.inf))
    near = ~c.lin & (c.mid >= -0.5) & (c.mid <= 1.5) & (np.hypot(T.ctr[ik, 0] - x[ip], T.ctr[ik, 1] - y[ip]) - T.rad[ik] <= reach[:M])
    with np.errstate(all="ignore"):
        dq = np.where(near, np.abs(_f(c.disc)) / c.sc_disc, np.inf)
    out.disc = np.full(P, np.inf)
    np.minimum.at(out.disc, ip, dq)
    return out


# ---- restricted margins for placing a point --------------------------------------------------------------------------------------
def group_best(T, ks, x, y):
    """(|d|, scale) of the best admissible root of the segments ks (a list) for points x, y; |d| = 1e300 where there is none"""
    best, scale = DD(np.full(x.shape, LD(1e300))), np.zeros(x.shape)
    for k in ks:
        c = candidates(T, np.full(x.shape, k), x, y)
        for r in (0, 1):
            take = c.adm[r] & np.asarray(c.ad[r] < best)
            best, scale = dd.where(take, c.ad[r], best), np.where(take, c.sc_d[r], scale)
    return best, scale


def margin_fn(T, kind, A, B=None, d_limit=None, edge=None):
    """g(x, y) -> (margin / scale) of one placed decision, arrays in, float64 out (its sign is exact: taken before the division).
    gap: best of group B - best of group A;  limit: d_limit - best of group A;  window: the ``edge`` ('lo' / 'hi') of segment A[0]'s
    root nearest to it."""
    def g(x, y):
        if kind == "gap":
            (a, sa), (b, sb) = group_best(T, A, x, y), group_best(T, B, x, y)
            return _f(b - a) / (sa + sb)
        if kind == "limit":
            a, sa = group_best(T, A, x, y)
            return _f(DD(LD(d_limit)) - a) / (d_limit + sa)
        c = candidates(T, np.full(x.shape, A[0]), x, y)
        w = c.wlo if edge == "lo" else c.whi
        r = np.where(c.have[1] & (np.abs(_f(w[1])) < np.abs(_f(w[0]))), 1, 0)
        return np.where(r == 1, _f(w[1]) / c.sc_w[1], _f(w[0]) / c.sc_w[0])
    return g


def place(g, p0, v, t0, t1, targets):
    """The doubles nearest to the edge g = 0 on the line p0 + t v, t0 < t < t1 (g changes sign there), displaced so that g comes
    as close as the lattice of doubles allows to each of ``targets`` (margin / scale, signed) -> [(x, y, g)] per target."""
    p0, v = np.asarray(p0, float), np.asarray(v, float)
    at = lambda t: (np.atleast_1d(p0[0] + t * v[0]), np.atleast_1d(p0[1] + t * v[1]))   # noqa: E731
    g0, g1 = float(g(*at(t0))[0]), float(g(*at(t1))[0])
    assert g0 * g1 < 0, ("no sign change", g0, g1)
    for _ in range(80):
        tm = 0.5 * (t0 + t1)
        if tm == t0 or tm == t1:
            break
        gm = float(g(*at(tm))[0])
        if gm * g0 > 0:
            t0 = tm
        else:
            t1 = tm
    ts = 0.5 * (t0 + t1)
    h = 1e-4
    slope = (float(g(*at(ts + h))[0]) - float(g(*at(ts - h))[0])) / (2 * h)
    out = []
    ii, jj = (q.ravel() for q in np.meshgrid(np.arange(-7, 8), np.arange(-7, 8)))
    for target in targets:
        cx, cy = at(ts + target / slope)
        for _ in range(2):   # (a step along the line lands beside the target; walk the lattice of doubles around it)
            xs, ys = cx[0] + ii * np.spacing(abs(cx[0])), cy[0] + jj * np.spacing(abs(cy[0]))
            gs = g(xs, ys)
            best = int(np.argmin(np.abs(gs - target)))
            cx, cy = np.array([xs[best]]), np.array([ys[best]])
        out.append((float(xs[best]), float(ys[best]), float(gs[best])))
    return out


def _targets(kind):
    b = BAND[kind] * U
    return [(lvl, sign, sign * (f * b if f else rel)) for lvl, f, rel in LEVELS for sign in (1, -1)]


# ---- the case table --------------------------------------------------------------------------------------------------------------
def _normal_point(T, k, lam, d):
    """the double point at (segment k, lam, d) of the path's own frame (double arithmetic: a starting point, nothing more)"""
    p = T.path
    tan = frontend.compute_vertex_tangents(p.ref)
    t = tan[k] + lam * (tan[k + 1] - tan[k])
    t = t / math.hypot(*t)
    foot = p.ref[k] + lam * (p.ref[k + 1] - p.ref[k])
    return foot + d * np.array([-t[1], t[0]]), np.array([-t[1], t[0]]), t


def _specs(name):
    """What is placed on a path: (family, kind, label, dict for margin_fn, p0, v, t0, t1, d_limit).  The geometry is written for the
    unfilled path; the tail lies straight on behind the last vertex and only the ends family looks at it."""
    T = tables(name, VARIANTS[0] if name != "two" else None)
    out = []
    if name == "u":       # legs: segments 0..5 and 12..17, the bend 6..11
        for k, lam in ((1, 0.3), (3, 0.71), (5, 0.85)):   # (the last: inside the bend, the legs' last and first segments, no neighbours)
            p0, nrm, _ = _normal_point(T, k, lam, 0.0)
            out.append(("medial", "gap", f"legs_k{k}", dict(A=list(range(0, 6)), B=list(range(12, 18))), p0, nrm, 1.0, 2.5, 20.0))
        p0, nrm, _ = _normal_point(T, 2, 0.4, 0.0)   # 1.5 m from the first leg, the second leg's candidate at the limit of 2 m
        out.append(("limit", "limit", "runner_at_limit", dict(A=list(range(12, 18)), d_limit=2.0), p0, nrm, 1.0, 1.9, 2.0))
        for dl in (2.0, 0.5):
            p0, nrm, _ = _normal_point(T, 3, 0.37, 0.0)
            out.append(("limit", "limit", f"outer_{dl}", dict(A=[2, 3, 4], d_limit=dl), p0, -nrm, 0.5 * dl, 1.5 * dl, dl))
    if name == "serp":    # run j: segments 5 j .. 5 j + 2
        for j in (0, 5, 10):
            p0, nrm, _ = _normal_point(T, 5 * j + 1, 0.37, 0.0)
            sgn = 1.0 if j % 2 == 0 else -1.0
            out.append(("medial", "gap", f"runs_{j}_{j + 1}", dict(A=[5 * j, 5 * j + 1, 5 * j + 2], B=[5 * j + 5, 5 * j + 6, 5 * j + 7]), p0, sgn * nrm,
                        1.0, 3.0, 20.0))
        p0, nrm, _ = _normal_point(T, 1, 0.6, 0.0)
        out.append(("limit", "limit", "below_first_run_0.5", dict(A=[0, 1, 2], d_limit=0.5), p0, -nrm, 0.2, 0.9, 0.5))
    if name == "arc25":
        n0 = len(_base(name)) - 1
        p0, nrm, _ = _normal_point(T, n0 // 2, 0.3, 0.0)
        dl = 20.0
        out.append(("limit", "limit", f"outside_{dl}", dict(A=list(range(n0 // 2 - 2, n0 // 2 + 3)), d_limit=dl), p0, -nrm, 0.5 * dl, 1.5 * dl, dl))
    if name == "straight":
        for k in (20, 40, 61):
            p0, nrm, _ = _normal_point(T, k, 0.45, 0.0)
            out.append(("limit", "limit", f"beside_k{k}_20", dict(A=[k - 1, k, k + 1], d_limit=20.0), p0, nrm if k != 40 else -nrm, 15.0, 25.0, 20.0))
    if name == "two":
        p0, nrm, _ = _normal_point(T, 0, 0.5, 0.0)
        out.append(("limit", "limit", "beside_20", dict(A=[0], d_limit=20.0), p0, nrm, 15.0, 25.0, 20.0))
    # ends: behind the first and beyond the last vertex, |d| <= 1 m
    # (not the U: its far leg and the tail lie beside its first vertex; not at 3e6: the doubles there are 2e-9 segments apart)
    if name in ("arc25", "two", "scurve", "straight"):
        for variant in ((None,) if name == "two" else VARIANTS):
            Tv = tables(name, variant)
            last = Tv.n_seg - 1
            for k, lam, edge, dside in ((0, 0.0, "lo", 0.6), (last, 1.0, "hi", -0.9), (0, 0.0, "lo", -0.05)):
                if k == 0 and variant == VARIANTS[1]:
                    continue   # (the first vertex is the same in both tables)
                p0, nrm, t = _normal_point(Tv, k, lam, dside)
                ln = math.hypot(*(Tv.path.ref[k + 1] - Tv.path.ref[k]))
                out.append(("ends", "window", f"{'first' if edge == 'lo' else 'last'}_{dside}_n{Tv.n_seg}", dict(A=[k], edge=edge, variant=variant), p0, t,
                            -3e-12 * ln if edge == "lo" else -1e-3 * ln, 1e-3 * ln if edge == "lo" else 3e-12 * ln, 20.0))
    return out


def _medial_groups(T, spec_kw, p0):
    """group B of an inside-of-the-bend case: the segments across the bend (those that are no neighbours of group A)"""
    if spec_kw.get("B") is not None:
        return spec_kw["A"], spec_kw["B"]
    A = spec_kw["A"]
    n0 = len(_base(T.path.name)) - 1
    return A, [k for k in range(n0) if k < A[0] - 6 or k > A[-1] + 6]


@functools.lru_cache(maxsize=None)
def placed(name):
    """The placed cases of one path: list of namespaces (family, kind, label, level, sign, x, y, d_limit, variant (None: both tables),
    g: the placed margin over its scale as the restricted evaluation gave it)."""
    rows = []
    for family, kind, label, kw, p0, v, t0, t1, d_limit in _specs(name):
        kw = dict(kw)
        variant = kw.pop("variant", VARIANTS[0] if name != "two" else None)
        T = tables(name, variant)
        if kind == "gap":
            kw["A"], kw["B"] = _medial_groups(T, kw, p0)
            A, B = kw["A"], kw["B"]
            if min(B) < min(A):      # the margin is (later group) - (earlier group): >= 0 keeps the first
                kw["A"], kw["B"] = B, A
        g = margin_fn(T, kind, **kw)
        tg = _targets(kind)
        for (lvl, sign, _), (x, y, gv) in zip(tg, place(g, p0, v, t0, t1, [t[2] for t in tg])):
            rows.append(NS(path=name, family=family, kind=kind, label=label, level=lvl, sign=sign, x=x, y=y, d_limit=d_limit, g=gv,
                           variant=variant if family == "ends" and name != "two" and label.startswith("last") else None))
    return rows


def _vnormal(name):
    """Points on the normal through interior vertices, both sides, |d| from 0 to 15 m (inside the bend: up to 0.8 radius)"""
    T = tables(name, VARIANTS[0])
    n0 = len(_base(name)) - 1
    ks = {"arc6": (20, 40, 77, 100), "scurve": (30, 60, 61, 70, 79, 80, 110), "u": (3, 6, 9), "straight": (10, 40, 41)}[name]
    inner = {"arc6": 4.8, "scurve": 7.0, "u": 1.4, "straight": 15.0}[name]
    rows = []
    for k in ks:
        assert 0 < k < n0
        kink = name == "scurve" and k in (60, 61, 70, 79, 80)   # (a 0.5 m segment meets a 0.01 m one: the tangent turns 0.02 rad within 0.01 m,
        for d in (0.0, 1e-3, -1e-3, 0.2, -0.2) if kink else (0.0, 1e-3, -1e-3, 0.5, -0.5, 3.0, -3.0, 15.0, -15.0):   # the normals cross 0.45 m inside)
            side = {"arc6": 1, "scurve": 0, "u": 1, "straight": 0}[name]       # the side the path bends to (0: both, mildly)
            if side == 0 or d * side > 0:
                d = math.copysign(min(abs(d), inner), d)
            p, _, _ = _normal_point(T, k, 0.0, d)
            rows.append(NS(path=name, family="vnormal", kind=None, label=f"v{k}_d{d}", level="", sign=0, x=float(p[0]), y=float(p[1]), d_limit=20.0,
                           g=math.nan, variant=None, vertex=k))
    return rows


def _straight():
    T = tables("straight", VARIANTS[0])
    rng = np.random.default_rng(7)
    rows = []
    for k in range(0, 81):
        for d in (rng.uniform(-3.0, 3.0), rng.uniform(-0.2, 0.2)):
            p, _, _ = _normal_point(T, k, float(rng.uniform(0.05, 0.95)), float(d))
            rows.append(NS(path="straight", family="straight", kind=None, label=f"k{k}", level="", sign=0, x=float(p[0]), y=float(p[1]), d_limit=20.0,
                           g=math.nan, variant=None))
    return rows


def _ties(name):
    """Exactly tied points (y midway between runs that carry the same x, dyadic x inside interior segments) and untied ones, alternating"""
    rows = []
    if name == "u_axis":
        xs = 0.5 + np.arange(14) * 0.515625
        spots = [(float(x), 2.0) for x in xs]
    elif name == "serp":
        spots = [(-500.0 + 8.25 + 0.484375 * i, 500.0 + 4.0 * (i % 11) + 2.0) for i in range(16)]
    else:   # laps: 2, 3 and 11 tied runs
        spots = [(53.0 + 0.03125 * i, 2.0) for i in range(40)] + [(29.0 + 0.15625 * i, 2.0) for i in range(60)] + [(8.5 + 0.109375 * i, 2.0) for i in range(60)]
    for i, (x, y) in enumerate(spots):
        rows.append(NS(path=name, family="ties", kind=None, label=f"tie{i}", level="tied", sign=0, x=x, y=y, d_limit=20.0, g=0.0, variant=None))
        off = (x, y + (0.75 if i % 2 else -0.625))
        if name == "laps":   # (beside runs that lie on each other every point is tied: the untied ones sit below the one run that is alone)
            off = (50.5 + 0.03125 * i, -1.0 - 0.25 * (i % 3))
        rows.append(NS(path=name, family="ties", kind=None, label=f"off{i}", level="untied", sign=0, x=off[0], y=off[1], d_limit=20.0, g=math.nan,
                       variant=None))
    return rows


def _listedge():
    """Points 1 m below the nine stacked runs: exactly nine open segments (one more than a lane lists), the winner on the LAST of them"""
    rows = []
    for i in range(70):
        rows.append(NS(path="stack", family="listedge", kind=None, label=f"nine{i}", level="nine", sign=0, x=9.5 + 0.0703125 * i, y=-1.0 - 0.0078125 * (i % 5),
                       d_limit=20.0, g=math.nan, variant=None))
    return rows


def _exact_limit(name):
    """The tied points again with d_limit = 2.0 = their |d|, every operation exact: inside, by ``<=``"""
    return [NS(path=name, family="limit", kind=None, label="at_limit_" + r.label, level="exact", sign=1, x=r.x, y=r.y, d_limit=2.0, g=0.0, variant=None)
            for r in _ties(name) if r.level == "tied"][:16]


@functools.lru_cache(maxsize=None)
def _focal(name):
    """Points inside the bend at 1.2 to 3 radii from the path (beyond the centre): most segments hold an admissible root, some two, and
    disc changes sign nearby.  The one family that SELECTS: a drawn point is admitted where the truth's winner leads by >= 8 B (and no
    disc and no root that matters is nearer than that to its edge)."""
    T = tables(name, VARIANTS[0])
    rng = np.random.default_rng([5, PATHS.index(name)])
    if name == "scurve":   # where a 0.5 m segment meets a 0.01 m one the tangent turns 0.02 rad within 0.01 m: a caustic 0.45 m inside, where
        pts = np.array([_normal_point(T, (60, 79)[q % 2], float(rng.uniform(0, 1)), -float(rng.uniform(0.3, 0.7)))[0] for q in range(FOCAL_TRIED)])   # disc changes sign
        return _focal_rows(name, pts)
    if name == "u_axis":   # inside the 45-90-45 degree corners of the U: |a| = 0.6 |e| on the joints, both roots near the window, disc of either sign
        return _focal_rows(name, np.stack((rng.uniform(13.0, 17.9, FOCAL_TRIED), rng.uniform(0.3, 3.7, FOCAL_TRIED)), 1))
    R = 6.0 if name == "arc6" else 25.0
    n0 = len(_base(name)) - 1
    # Every other draw lies within 1.5 sagittas (2 mm) of the centre: the vertex normals of a regular polygon all pass through it and a
    # segment's normals fan out by its sagitta there -- that is where most segments hold a root.  A point farther away lies on two normals
    # of the bend, no more: the draws at 1.2 to 3 radii hold the far side's candidate against the near side's.
    centre = {"arc6": _rot([[0.0, R]], 0.7, (3.0e6, -2.1e6)), "arc25": _rot([[0.0, R]], -0.4, (0.0, 0.0))}[name][0]
    sag = R * (1.0 - math.cos(0.5 * (0.25 if name == "arc6" else 0.5) / R))
    pts = []
    for q in range(FOCAL_TRIED):
        if q % 2 == 0:
            rho, phi = 1.5 * sag * math.sqrt(rng.uniform()), rng.uniform(0.0, 2.0 * math.pi)
            pts.append(centre + rho * np.array([math.cos(phi), math.sin(phi)]))
        else:
            pts.append(_normal_point(T, int(rng.integers(2, n0 - 2)), float(rng.uniform(0, 1)), float(rng.uniform(1.2, 3.0)) * R)[0])
    return _focal_rows(name, np.array(pts))


def _focal_rows(name, pts):
    t = exact(name, VARIANTS[0], pts[:, 0], pts[:, 1], FOCAL_LIMIT[name])
    ok = t.inside & (t.gap >= DECIDED * BAND["gap"] * U) & (t.disc >= DECIDED * BAND["gap"] * U) & (t.window >= DECIDED * BAND["window"] * U)
    level = lambda i: "caustic" if name == "scurve" else "corner" if name == "u_axis" else "centre" if i % 2 == 0 else "beyond"   # noqa: E731
    return [NS(path=name, family="focal", kind=None, label=f"f{i}", level=level(i), sign=0, x=float(pts[i, 0]), y=float(pts[i, 1]), d_limit=FOCAL_LIMIT[name],
               g=math.nan, variant=None) for i in np.flatnonzero(ok)]


@functools.lru_cache(maxsize=None)
def cases(name):
    """Every case of one path, in the order in which the batches interleave them"""
    rows = list(placed(name))
    if name in ("arc6", "scurve", "u", "straight"):
        rows += _vnormal(name)
    if name == "straight":
        rows += _straight()
    if name in FOCAL_LIMIT:
        rows += _focal(name)
    if name == "stack":
        rows += _listedge()
    if name in ("u_axis", "serp", "laps"):
        rows += _ties(name)
    if name in ("u_axis", "serp"):
        rows += _exact_limit(name)
    fams = sorted({r.family for r in rows})
    by = {f: [r for r in rows if r.family == f] for f in fams}
    mixed = []   # neighbouring lanes hold different families
    while any(by.values()):
        for f in fams:
            if by[f]:
                mixed.append(by[f].pop(0))
    return tuple(mixed)


@functools.lru_cache(maxsize=None)
def batch(name, variant):
    """The cases of a path that run on the table ``variant`` (a row count, None for ``two``), grouped by d_limit: {d_limit: namespace
    (rows, x, y, theta, truth, oracle)}.  theta: the truth's path heading at the winner + 0.1 rad (0 outside)."""
    out = {}
    rows = [r for r in cases(name) if r.variant in (None, variant)]
    p = path(name, variant)
    for dl in sorted({r.d_limit for r in rows}):
        sel = [r for r in rows if r.d_limit == dl]
        x, y = np.array([r.x for r in sel]), np.array([r.y for r in sel])
        t = exact(name, variant, x, y, dl)
        k = np.maximum(t.seg, 0)
        theta = np.where(t.inside, p.theta[k] + _f(t.lam) * (p.theta[k + 1] - p.theta[k]) + 0.1, 0.0)
        t = exact(name, variant, x, y, dl, theta)
        s, d, seg, lam = S.project_batch(p.ref, p.pos, x, y, dl)
        numpy_sd = (s, d)
        _, s, d = doubles(p, x, y, dl, which=("oracle",))["oracle"]     # (s and d of the value rule: oracle.frontend.project's own)
        with np.errstate(invalid="ignore"):
            th = S.valid_orientation(theta - (p.theta[np.maximum(seg, 0)] + lam * (p.theta[np.maximum(seg, 0) + 1] - p.theta[np.maximum(seg, 0)])))
        for q in (x, y, theta):
            q.setflags(write=False)
        out[dl] = NS(rows=sel, x=x, y=y, theta=theta, truth=t, oracle=NS(s=s, d=d, seg=seg, theta_cl=np.where(seg >= 0, th, np.nan)),
                     numpy=NS(s=numpy_sd[0], d=numpy_sd[1], seg=seg), path=p, d_limit=dl)
    return out


def variants_of(name):
    return (None,) if name == "two" else VARIANTS


def all_batches():
    for name in PATHS:
        for variant in variants_of(name):
            for dl, b in batch(name, variant).items():
                yield name, variant, dl, b


def placed_margin(b):
    """the placed margin over its scale of every row of a batch, from the FULL truth (NaN: the row places none)"""
    t = b.truth
    out = np.full(len(b.rows), np.nan)
    for i, r in enumerate(b.rows):
        if r.kind == "gap":
            first = t.seg[i] < t.runner_seg[i]
            out[i] = t.gap[i] if first else -t.gap[i]
        elif r.kind == "limit":
            out[i] = t.limit[i] * r.sign     # (unsigned in the truth: the sign is checked through the verdict below)
        elif r.kind == "window":
            out[i] = t.window[i] * r.sign
    return out


def admission_failures(b):
    """Rows of a batch that do not meet the conditions of a case (empty: all do)"""
    t, bad = b.truth, []
    pm = placed_margin(b)
    for i, r in enumerate(b.rows):
        others = {"gap": t.gap[i], "limit": t.limit[i], "window": t.window[i], "disc": t.disc[i]}
        if r.level == "exact":
            if not (t.inside[i] and t.limit[i] == 0.0 and t.gap_zero[i] and t.seg[i] < t.runner_seg[i]):
                bad.append((r.label, "not exactly at the limit", t.limit[i]))
            others.pop("gap"), others.pop("limit")
        elif r.family == "ties" and r.level == "tied":
            if not (t.gap_zero[i] and t.gap[i] == 0.0 and t.n_tied[i] >= 2 and t.seg[i] < t.runner_seg[i]):
                bad.append((r.label, "not an exact tie", t.gap[i]))
            others.pop("gap")
        elif r.family == "focal":                # (admitted by its gap alone: see _focal)
            if not (t.inside[i] and min(t.gap[i], t.disc[i], t.window[i]) >= DECIDED * BAND["gap"] * U):
                bad.append((r.label, "the winner does not lead by 8 B, or disc or a root is nearer to its edge", t.gap[i] / U, t.disc[i] / U, t.window[i] / U))
            others = {}
        elif r.family in ("vnormal", "straight"):
            others.pop("window")             # (vnormal: the two roots sit ON the window; straight: values only)
            if r.family == "vnormal" and not (t.inside[i] and t.seg[i] in (r.vertex - 1, r.vertex)):
                bad.append((r.label, "the truth is outside the domain, or elsewhere", int(t.seg[i])))
        elif r.kind is not None:
            others.pop(r.kind)
            if not (abs(pm[i]) >= DECIDED * BAND[r.kind] * U and np.sign(pm[i]) == r.sign):
                bad.append((r.label, r.level, r.sign, "placed margin", pm[i] / U))
            if r.kind == "limit" and r.label != "runner_at_limit" and bool(t.inside[i]) != (r.sign > 0):
                bad.append((r.label, r.level, r.sign, "inside" if t.inside[i] else "outside"))
            if r.kind == "window" and bool(t.inside[i]) != (r.sign > 0):
                bad.append((r.label, r.level, r.sign, "inside" if t.inside[i] else "outside"))
        for kind, v in others.items():
            need = OTHER_UNPLACED * BAND.get(kind, 64.0) * U if r.family in ("vnormal", "straight") else OTHER
            if not v >= need:
                bad.append((r.label, r.level, r.sign, "other margin", kind, v))
    return bad


# ---- the three double implementations ------------------------------------------------------------------------------------------
def doubles(p, x, y, d_limit, which=("oracle", "numpy", "host")):
    """{name: (inside [P], s [P], d [P])} of oracle.frontend.project, tests/_score.project_batch and the host rp_project"""
    from commonroad_rp_amd import _capi
    out = {}
    if "numpy" in which:
        s, d, seg, _ = S.project_batch(p.ref, p.pos, x, y, d_limit)
        out["numpy"] = (seg >= 0, s, d)
    for key in ("oracle", "host"):
        if key not in which:
            continue
        ins, s, d = np.zeros(len(x), bool), np.full(len(x), np.nan), np.full(len(x), np.nan)
        for i in range(len(x)):
            if key == "oracle":
                r = frontend.project(p.ref, p.pos, float(x[i]), float(y[i]), d_limit)
            else:
                try:
                    r = _capi.project(p.ref, p.pos, float(x[i]), float(y[i]), d_limit)
                except ValueError:
                    r = None
            if r is not None:
                ins[i], s[i], d[i] = True, r[0], r[1]
        out[key] = (ins, s, d)
    return out


def same_decision(t, impl):
    """[P]: the implementation is inside where the truth is, and its s is the truth's (to 1e-4 m: the other outcome is metres away)"""
    ins, s, _ = impl
    with np.errstate(invalid="ignore"):
        return (ins == t.inside) & (~t.inside | (np.abs(s - _f(t.s)) <= 1e-4))


@functools.lru_cache(maxsize=None)
def measure():
    """{kind: (draws, worst |margin| / (u scale) at which a double implementation decided otherwise than the truth)}.  The draws: the
    doubles of a 25 x 25 lattice around every placed case's edge whose margin lies within 2^12 u scale."""
    res = {k: [0, 0.0] for k in KINDS}
    ii, jj = (q.ravel() for q in np.meshgrid(np.arange(-12, 13), np.arange(-12, 13)))
    for name in PATHS:
        for family, kind, label, kw, p0, v, t0, t1, d_limit in _specs(name):
            kw = dict(kw)
            variant = kw.pop("variant", VARIANTS[0] if name != "two" else None)
            T = tables(name, variant)
            if kind == "gap":
                kw["A"], kw["B"] = _medial_groups(T, kw, p0)
                if min(kw["B"]) < min(kw["A"]):
                    kw["A"], kw["B"] = kw["B"], kw["A"]
            g = margin_fn(T, kind, **kw)
            (x0, y0, _), = place(g, p0, v, t0, t1, [0.0])
            xs, ys = x0 + ii * np.spacing(abs(x0)), y0 + jj * np.spacing(abs(y0))
            gs = g(xs, ys)
            near = np.flatnonzero(np.abs(gs) <= 4096 * U)
            near = near[np.argsort(np.abs(gs[near]))]
            pick = np.unique(np.concatenate((near[:12], near[12::9][:12])))   # the twelve nearest to the edge, and a ladder outwards
            if not pick.size:
                continue
            xs, ys = xs[pick], ys[pick]
            t = exact(name, variant, xs, ys, d_limit)
            m = {"gap": t.gap, "limit": t.limit, "window": t.window}[kind]
            for impl in doubles(path(name, variant), xs, ys, d_limit).values():
                wrong = ~same_decision(t, impl)
                res[kind][0] += len(xs)
                if wrong.any():
                    res[kind][1] = max(res[kind][1], float(m[wrong].max() / U))
    return {k: tuple(v) for k, v in res.items()}


# ---- lift and back ---------------------------------------------------------------------------------------------------------------
LIFT_PATHS = ("arc25", "scurve")
LIFT_D = (0.0, 0.25, -0.25, 1.5, -1.5, 0.03125, -3.0)


def lift_exact(name, variant, s, d, d_limit):
    """include/rp_lift.h's point rule: the segment and the on-path verdict by comparisons of the doubles (no guard: none is needed),
    the position in double-word arithmetic -> namespace on, seg (-1 off the path), x, y (longdouble, NaN off the path), x_dd, y_dd"""
    T = tables(name, variant)
    pos = T.path.pos
    s, d = np.asarray(s, float), np.asarray(d, float)
    on = np.isfinite(s) & np.isfinite(d) & (pos[0] <= s) & (s <= pos[-1]) & (np.abs(d) <= d_limit)
    k = np.clip(np.searchsorted(pos, np.where(on, s, pos[0]), side="right") - 1, 0, len(pos) - 2)
    S_, D_ = DD(_ld(np.where(on, s, pos[0]))), DD(_ld(np.where(on, d, 0.0)))
    lam = (S_ - T.pos0[k]) / T.dpos[k]
    tx, ty = T.t0x[k] + lam * T.dtx[k], T.t0y[k] + lam * T.dty[k]
    tn = dd.sqrt(tx * tx + ty * ty)
    x, y = (T.px[k] + lam * T.ex[k]) - D_ * (ty / tn), (T.py[k] + lam * T.ey[k]) + D_ * (tx / tn)
    nan = LD(np.nan)
    return NS(on=on, seg=np.where(on, k, -1), x=np.where(on, x.ld(), nan), y=np.where(on, y.ld(), nan), x_dd=x, y_dd=y)


@functools.lru_cache(maxsize=None)
def lift_batch(name, variant):
    """(s, d) with s on every vertex of the table, one double on either side of it (at ref_pos[0] and ref_pos[-1]: one inside, one
    OUTSIDE), d cycling through LIFT_D; the exact lift; the oracle's lift (tests/_lift.point) and its way back (tests/_score.project_batch);
    and ``unique``: the exact projection of the exactly lifted point, rounded to doubles, is (s, d) again with no other candidate
    within 1e-6 scale of it -- there the way back is held to the value rule."""
    import _lift
    p = path(name, variant)
    s = np.stack((np.nextafter(p.pos, -np.inf), p.pos, np.nextafter(p.pos, np.inf)), 1).ravel()
    d = np.resize(LIFT_D, s.size)
    d_limit = 20.0
    t = lift_exact(name, variant, s, d, d_limit)
    lt = NS(ref=p.ref, pos=p.pos, d_limit=d_limit, tan=frontend.compute_vertex_tangents(p.ref))
    ox, oy, oseg = _lift.points(lt, s, d)
    xr, yr = to_double(dd.where(t.on, t.x_dd, dd.zeros(s.shape))), to_double(dd.where(t.on, t.y_dd, dd.zeros(s.shape)))
    back = exact(name, variant, xr, yr, d_limit)
    sc = np.abs(xr) + np.abs(yr) + np.abs(s)
    with np.errstate(invalid="ignore"):
        unique = t.on & back.inside & (back.gap >= OTHER) & (back.limit >= OTHER) & (np.abs(_f(back.s) - s) <= 1e-9 * sc) & (np.abs(_f(back.d) - d) <= 1e-9 * sc)
    bs, bd, bseg, _ = S.project_batch(p.ref, p.pos, np.where(t.on, ox, np.nan), np.where(t.on, oy, np.nan), d_limit)
    for q in (s, d):
        q.setflags(write=False)
    return NS(path=p, s=s, d=d, d_limit=d_limit, truth=t, unique=unique, oracle=NS(x=ox, y=oy, seg=oseg, s=bs, d=bd, back_seg=bseg))


def lift_failures(lb, x, y, seg, n_outside, s_back, d_back):
    """What a lift (x, y, seg, n_outside) and the projection of ITS points (s_back, d_back) miss on a lift batch: the verdicts exactly,
    the positions by the value rule against the double-word lift, and (s, d) back by the value rule against the (s, d) that went in, over
    the unique points.  ``s_back`` None: the lift alone."""
    t, out = lb.truth, []
    if not (np.array_equal(seg, t.seg) and np.array_equal(np.isnan(x), ~t.on) and np.array_equal(np.isnan(y), ~t.on) and n_outside == int((~t.on).sum())):
        out.append(f"{lb.path.name}: segment or on-path verdict at {np.flatnonzero((seg != t.seg) | (np.isnan(x) == t.on))[:8]}")
        return out
    rows = [("x", t.x, lb.oracle.x, x, t.on), ("y", t.y, lb.oracle.y, y, t.on)]
    if s_back is not None:
        with np.errstate(invalid="ignore"):
            same = lb.unique & (np.abs(lb.oracle.s - lb.s) <= 1e-4)
        rows += [("s back", lb.s.astype(LD), lb.oracle.s, s_back, same), ("d back", lb.d.astype(LD), lb.oracle.d, d_back, same)]
    for row, truth, orc, dev, sel in rows:
        eo, ed, bound, ro, rd, rbound = value_rule(truth, orc, dev, sel)
        if not (ed <= bound and rd <= rbound):
            out.append(f"{lb.path.name} {row}: E_O {eo:.3e} E_D {ed:.3e} bound {bound:.3e}; R_O {ro:.3e} R_D {rd:.3e} bound {rbound:.3e} over {int(sel.sum())}")
    return out


# ---- the documented double arithmetic, with planted defects ----------------------------------------------------------------------
DEFECTS = ("le_for_lt", "lt_at_limit", "window_0", "textbook_root", "second_root_dropped", "disc_gt_0")


def restated(p, x, y, d_limit, defect=None, near=None):
    """rpfe::project (csrc/rp_frontend.h) in NumPy doubles over points x, y [P] -> namespace s, d, seg, lam.  ``defect``: one of DEFECTS.
    ``near`` [P]: only the segments near - 1, near, near + 1 of each point (with the WHOLE path's vertex tangents)."""
    ref, pos = p.ref, p.pos
    P = len(x)
    tan = frontend.compute_vertex_tangents(ref)
    s, d, lam_out, seg = np.full(P, np.nan), np.full(P, np.nan), np.full(P, np.nan), np.full(P, -1)
    lo, hi = (0.0, 1.0) if defect == "window_0" else (-1e-12, 1.0 + 1e-12)
    with np.errstate(all="ignore"):
        for k in range(len(ref) - 1):
            ex, ey = ref[k + 1] - ref[k]
            qx, qy = x - ref[k, 0], y - ref[k, 1]
            t0x, t0y = tan[k]
            dtx, dty = tan[k + 1] - tan[k]
            a = -(ex * dtx + ey * dty)
            b = (qx * dtx + qy * dty) - (ex * t0x + ey * t0y)
            c = qx * t0x + qy * t0y
            if abs(a) < 1e-14:
                roots = [np.where(b != 0.0, -c / b, np.nan)]
            else:
                disc = b * b - 4.0 * a * c
                none = disc <= 0.0 if defect == "disc_gt_0" else disc < 0.0
                sq = np.sqrt(np.where(none, np.nan, disc))
                if defect == "textbook_root" and abs(a) < 1e-10:
                    roots = [(-b + sq) / (2.0 * a), (-b - sq) / (2.0 * a)]
                else:
                    bp = b >= 0.0
                    q = np.where(bp, -0.5 * (b + sq), -0.5 * (b - sq))
                    zero = q == 0.0
                    roots = [np.where(zero, 0.0, np.where(bp, c / q, q / a)), np.where(zero, 0.0, np.where(bp, q / a, c / q))]
                roots = [np.where(none, np.nan, r) for r in roots]
                if defect == "second_root_dropped":
                    roots = roots[:1]
            for lam in roots:
                adm = (lam >= lo) & (lam <= hi)
                lam = np.minimum(np.maximum(lam, 0.0), 1.0)
                tx, ty = t0x + lam * dtx, t0y + lam * dty
                fx, fy = ref[k, 0] + lam * ex, ref[k, 1] + lam * ey
                dd_ = (-(x - fx) * ty + (y - fy) * tx) / np.sqrt(tx * tx + ty * ty)
                within = np.abs(dd_) < d_limit if defect == "lt_at_limit" else np.abs(dd_) <= d_limit
                better = np.abs(dd_) <= np.abs(d) if defect == "le_for_lt" else np.abs(dd_) < np.abs(d)
                take = adm & within & ((seg < 0) | better)
                if near is not None:
                    take = take & (np.abs(k - near) <= 1)
                s, d, lam_out, seg = np.where(take, pos[k] + lam * (pos[k + 1] - pos[k]), s), np.where(take, dd_, d), np.where(take, lam, lam_out), np.where(take, k, seg)
    return NS(s=s, d=d, seg=seg, lam=lam_out)


@functools.lru_cache(maxsize=None)
def disc_zero_cases():
    """(path, x, y): points whose disc is 0.0 IN DOUBLES on segment 0 of a three-vertex path with a sharp joint (a = 0.30), the double
    root inside the window and the only candidate -- found on the lattice of doubles around the curve b^2 = 4 a c.  Rows of the
    DOCUMENTED arithmetic (b * b - 4.0 * a * c, each operation rounded), not of the truth: the real disc there is +-1e-16, below every
    guard band, and a fused multiply-add decides it either way -- so these rows hold the NumPy restatement alone, never the device."""
    ref = np.array([[0.0, 0.0], [4.0, 0.0], [4.5, 0.5]])
    p = NS(name="joint", ref=ref, pos=frontend.compute_pathlength_from_polyline(ref))
    tan = frontend.compute_vertex_tangents(ref)
    (ex, ey), (t0x, t0y), (dtx, dty) = ref[1] - ref[0], tan[0], tan[1] - tan[0]
    a = -(ex * dtx + ey * dty)
    ii, jj = (q.ravel() for q in np.meshgrid(np.arange(-40, 41), np.arange(-40, 41)))
    xs, ys = [], []
    for lam0 in np.linspace(0.2, 0.8, 25):
        b0 = -2.0 * a * lam0
        qx = b0 * b0 / (4.0 * a)
        qy = (b0 + (ex * t0x + ey * t0y) - qx * dtx) / dty
        x, y = qx + ii * np.spacing(qx), qy + jj * np.spacing(qy)
        b = (x * dtx + y * dty) - (ex * t0x + ey * t0y)
        hit = np.flatnonzero(b * b - 4.0 * a * (x * t0x + y * t0y) == 0.0)[:2]
        xs += list(x[hit])
        ys += list(y[hit])
    return p, np.array(xs), np.array(ys)


# ---- what the device's pruning makes of the inputs -------------------------------------------------------------------------------
def open_counts(p, x, y, d_limit):
    """Per point the number of segments the pruned walk lists (csrc/rp_score.hip, project_pose), in doubles: the bound U is the best
    candidate of the nearest circle's segment and its neighbours (none: d_limit), a segment is open when dist^2 <= (r + U)^2 * 1.000001."""
    e = np.diff(p.ref, axis=0)
    ctr = p.ref[:-1] + 0.5 * e
    rad = 0.5 * np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) * (1.0 + 1e-12)
    d2 = (ctr[None, :, 0] - x[:, None]) ** 2 + (ctr[None, :, 1] - y[:, None]) ** 2
    kn = np.argmin(d2, axis=1)
    u = restated(p, x, y, d_limit, near=kn)
    bound = np.where(u.seg >= 0, np.abs(u.d), float(d_limit))
    sm = rad[None] + bound[:, None]
    return (d2 <= sm * sm * 1.000001).sum(axis=1)


# ---- the value rule (that of tests/_xref.py) ---------------------------------------------------------------------------------------
def value_rule(truth_row, oracle_row, device_row, sel):
    """(e_o, e_d, bound, r_o, r_d, rms bound) of one row (s, d or theta_cl) of one batch over the elements sel"""
    if not sel.any():
        return 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    X = np.asarray(truth_row)[sel]
    eo = np.abs(np.asarray(oracle_row)[sel].astype(LD) - X).astype(np.float64)
    ed = np.abs(np.asarray(device_row)[sel].astype(LD) - X).astype(np.float64)
    ed = np.where(np.isfinite(ed), ed, np.inf)
    sp = float(np.spacing(np.abs(X).max().astype(np.float64)))
    rms = lambda q: float(np.sqrt((q * q).mean()))   # noqa: E731
    return (float(eo.max()), float(ed.max()), MARGIN_MAX * float(eo.max()) + FLOOR_MAX * sp, rms(eo), rms(ed), MARGIN_RMS * rms(eo) + FLOOR_RMS * sp)


def comparable(b):
    """rows of a batch whose values the rule compares: inside, and the oracle took the truth's candidate (on a vertex normal the twin
    segment's root is the same point)"""
    with np.errstate(invalid="ignore"):
        return b.truth.inside & (b.oracle.seg >= 0) & (np.abs(b.oracle.s - _f(b.truth.s)) <= 1e-4)


def decision_failures(b, got):
    """Rows of a batch on which ``got`` (namespace: s, d [P]; seg [P] or None) decides otherwise than the truth: the NaN pattern, the
    candidate (its s to 1e-4 m: another candidate is metres away), the segment where ``got`` has one (on a vertex normal: k - 1 or k),
    s at the path's end for the ends family, and s and d bit for bit on the exact rows."""
    t, bad = b.truth, []
    sx, dx = to_double(t.s_dd), to_double(t.d_dd)
    pos = b.path.pos
    for i, r in enumerate(b.rows):
        outside = bool(np.isnan(got.s[i]))
        if outside != bool(np.isnan(got.d[i])) or outside == bool(t.inside[i]) or (got.seg is not None and (got.seg[i] < 0) != outside):
            bad.append((i, r.family, r.label, r.level, r.sign, "outside" if outside else "inside"))
            continue
        if outside:
            continue
        if not abs(got.s[i] - float(t.s[i])) <= 1e-4:
            bad.append((i, r.family, r.label, r.level, r.sign, "another candidate", float(got.s[i]), float(t.s[i])))
            continue
        if got.seg is not None:
            ok = got.seg[i] in (r.vertex - 1, r.vertex) if r.family == "vnormal" else got.seg[i] == t.seg[i]
            if not ok:
                bad.append((i, r.family, r.label, r.level, r.sign, "segment", int(got.seg[i]), int(t.seg[i])))
        if r.family == "ends" and sx[i] in (pos[0], pos[-1]) and got.s[i] != sx[i]:
            bad.append((i, r.family, r.label, r.level, r.sign, "s is not the path's end", float(got.s[i])))
        if r.level in ("tied", "exact") and not (got.s[i] == sx[i] and got.d[i] == dx[i]):
            bad.append((i, r.family, r.label, r.level, r.sign, "not bit-equal", float(got.s[i]) - sx[i], float(got.d[i]) - dx[i]))
    return bad


def value_failures(b, got, rows=("s", "d", "theta_cl")):
    """Lines of the value rule that ``got`` exceeds on a batch, per family and row, over the rows that ``comparable`` names and on which
    got took the truth's candidate as well"""
    ok = comparable(b)
    with np.errstate(invalid="ignore"):
        ok = ok & (np.abs(got.s - _f(b.truth.s)) <= 1e-4)
    out = []
    for fam in sorted({r.family for r in b.rows}):
        sel = ok & np.array([r.family == fam for r in b.rows])
        for row in rows:
            eo, ed, bound, ro, rd, rbound = value_rule(getattr(b.truth, row), getattr(b.oracle, row), getattr(got, row), sel)
            if not (ed <= bound and rd <= rbound):
                out.append(f"{b.path.name} {fam} {row}: E_O {eo:.3e} E_D {ed:.3e} bound {bound:.3e}; R_O {ro:.3e} R_D {rd:.3e} bound {rbound:.3e}")
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------------
def main(out_file):
    lines = ["accuracy_projection: the curvilinear projection against the exact reference of tests/_proj.py", ""]
    if not HAVE_LONGDOUBLE:
        print(SKIP_REASON)
        return 1
    lines.append("guard band B = BAND u scale per decision kind; worst: the largest |margin| / (u scale) at which oracle.frontend.project,")
    lines.append("tests/_score.project_batch or the host rp_project decided otherwise than the reference, over the draws")
    for kind, (draws, worst) in measure().items():
        lines.append(f"  {kind:7s} BAND {BAND[kind]:6.0f}   worst {worst:8.3f}   draws {draws}")
    lines.append("  disc    borrows the gap band (the focal family admits a point only where every disc that matters keeps 8 B of it): no ladder is")
    lines.append("          drawn for it, since where disc is within a few u of 0 the pair of roots it decides is the segment's only pair and the")
    lines.append("          result hangs on one rounding of b * b - 4 a c, fused or not -- tests/test_proj_abi.py holds the documented arithmetic there")
    scorer = None
    try:
        import torch
        if torch.cuda.device_count() > 0:
            from commonroad_rp_amd import TrajectoryScorer
            scorer = TrajectoryScorer(0)
    except Exception as e:   # (no device: the table holds the oracle's columns alone)
        lines.append(f"(no device: {type(e).__name__})")
    lines += ["", "cases per family (built = admitted: tests/test_proj_abi.py asserts the conditions of a case for every one)"]
    count = {}
    for name, variant, dl, b in all_batches():
        if variant in (None, VARIANTS[0]):
            for r in b.rows:
                count[r.family] = count.get(r.family, 0) + 1
        else:
            for r in b.rows:
                if r.variant == variant:
                    count[r.family] = count.get(r.family, 0) + 1
    lines += [f"  {f:9s} {count.get(f, 0):5d}" for f in FAMILIES]
    lines += ["", f"focal family: {FOCAL_TRIED} points drawn per path, admitted where the reference's winner leads by >= 8 B"]
    lines.append("  open segments per lane (the list holds 8): only the draws at a bend's centre are many-segment lanes")
    for name in FOCAL_LIMIT:
        b = batch(name, VARIANTS[0])[FOCAL_LIMIT[name]]
        cnt = open_counts(b.path, b.x, b.y, FOCAL_LIMIT[name])
        for lvl in ("centre", "beyond", "caustic", "corner"):
            m = np.array([r.family == "focal" and r.level == lvl for r in b.rows])
            if m.any():
                lines.append(f"  {name:7s} {lvl:8s} admitted {int(m.sum()):4d}   open segments {int(cnt[m].min()):4d} .. {int(cnt[m].max()):4d}")
    lines += ["", "largest distance to the reference per family and row: oracle (E_O), device (E_D), the bound 8 E_O + 8 spacings", ""]
    worst = {}
    for name, variant, dl, b in all_batches():
        dev = None
        if scorer is not None:
            scorer.set_reference(b.path.ref, b.path.pos, b.path.theta, dl)
            o = scorer.score(S.fixture("cfg2_ref_draw").p, S.fixture("cfg2_ref_draw").cost, b.x[None], b.y[None], b.theta[None], v=np.ones((1, len(b.x))),
                             a=np.zeros((1, len(b.x))), kappa=np.zeros((1, len(b.x))), want_states=True)
            dev = dict(s=o.s[0], d=o.d[0], theta_cl=o.theta_cl[0])
        ok = comparable(b)
        for fam in sorted({r.family for r in b.rows}):
            sel = ok & np.array([r.family == fam for r in b.rows])
            for row in ("s", "d", "theta_cl"):
                tr = getattr(b.truth, row)
                eo, ed, bound, _, _, _ = value_rule(tr, getattr(b.oracle, row), dev[row] if dev else getattr(b.oracle, row), sel)
                w = worst.setdefault((fam, row), [0.0, 0.0, 0.0])
                w[0], w[1] = max(w[0], eo), max(w[1], ed if dev else 0.0)
                w[2] = max(w[2], (ed / bound) if dev and bound > 0 else 0.0)
    for (fam, row), (eo, ed, ratio) in sorted(worst.items()):
        lines.append(f"  {fam:9s} {row:9s} E_O {eo:9.3e}   E_D {ed:9.3e}   largest E_D / bound {ratio:6.3f}" if scorer else f"  {fam:9s} {row:9s} E_O {eo:9.3e}")
    lines += ["", "lift and back: (s, d) on and beside every vertex through the lift, the lifted points through the projection"]
    for name in LIFT_PATHS:
        for variant in VARIANTS:
            lb = lift_batch(name, variant)
            dev = None
            if scorer is not None:
                from commonroad_rp_amd import TrajectoryLifter
                with TrajectoryLifter(0) as lf:
                    zeros = np.zeros(len(lb.path.pos))
                    lf.set_reference(lb.path.ref, lb.path.pos, lb.path.theta, zeros, zeros, lb.d_limit)
                    dx, dy, _ = lf.points(lb.s, lb.d)
                scorer.set_reference(lb.path.ref, lb.path.pos, lb.path.theta, lb.d_limit)
                ds, dd_, _ = scorer.project(dx, dy)
                dev = dict(x=dx, y=dy, s=ds, d=dd_)
            for row, tr, orc, sel in (("x", lb.truth.x, lb.oracle.x, lb.truth.on), ("y", lb.truth.y, lb.oracle.y, lb.truth.on),
                                      ("s", lb.s.astype(LD), lb.oracle.s, lb.unique), ("d", lb.d.astype(LD), lb.oracle.d, lb.unique)):
                eo, ed, bound, _, _, _ = value_rule(tr, orc, dev[row] if dev else orc, sel)
                lines.append(f"  {name:7s} {variant} {row:2s} over {int(sel.sum()):5d}   E_O {eo:9.3e}" + (f"   E_D {ed:9.3e}   E_D / bound {ed / bound if bound else 0:6.3f}" if dev else ""))
    if scorer is not None:
        scorer.close()
    text = "\n".join(lines) + "\n"
    with open(out_file, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    _out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(S.REPO, "profiles", "accuracy_projection.txt")
    sys.exit(main(_out))
