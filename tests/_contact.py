"""Exact collision verdicts at near contact (TEST INFRASTRUCTURE: tests/test_contact_abi.py on the CPU, tests/test_contact.py on the GPU).
It shares nothing with oracle/rp_oracle.c, commonroad_rp_amd/collision.py or tests/_clearance.py.

TRUTH: the closed sets the DOUBLE inputs define, evaluated in double-word longdouble arithmetic (tests/_dd.py, about 128 bits).
  ego rectangle   centre = rear axle + wb_rear_axle (cos theta, sin theta), half extents length / 2, width / 2
  obstacle rows   as ObstacleTables takes them: rectangle (cx, cy, theta, hl, hw), triangle (x1 .. y3), circle (cx, cy, r)
  signed gap g    rectangle - rectangle: the maximum over the four unit axes of the separation |t . n| - (r_a(n) + r_b(n));
                  rectangle - triangle: the two rectangle axes and the unit normals of the non-degenerate edges (either vertex order);
                  rectangle - circle: distance of the centre to the rectangle (negative inside) minus r.        hit <=> g <= 0
  swept box       the rectangle around two consecutive ego rectangles, restated from its definition (the comment above merge_swept,
                  tests/golden/_ref_shims.py): the branch decisions are made here, and a case has to be 1e-3 away from either switch.
  distance        for the clearance query: the minimum vertex-to-segment distance, both ways (circle: g).

THE TABLE.  Every case is built by bisection along a contact direction in this reference, displaced along that direction by +- 64 B,
+- 2^16 B or +- 1e-6 m, its obstacle rounded to doubles, and the gap recomputed from those doubles: it must have the intended sign and
|g| >= 8 B -- a condition on the generator (asserted), never a reason to drop a case.  B = 8 u scale, u = 2^-53,
scale = |x| + |y| of the ego centre + the ego's bounding radius + the shape's bounding radius + the centre distance: 13 times the worst
error of the double predicate measured against this reference (0.61 u scale, profiles/accuracy_contact.txt).  Families:
  a  parallel edges (also a segment, hw = 0, parallel and perpendicular)      b  a corner into an edge, either way
  c  corner to corner with both diagonals on one line: the centre distance IS ego_r + r_bound, the bounding circles touch
  d  the diamond: only the obstacle's axes separate                           e  containment both ways (no displacement)
  f  strips hl = 40 m, hw = 0.05 and 0, touched at the far end (diagonal of the ego along the strip: the slab test is tight; along its
     normal: the normal test is tight) and at mid-length
  g  triangles: vertex on an edge, edge through a corner, collinear, clockwise, one with a 100 m edge
  h  circles: on an edge, on a corner, r = 0                                  i  swept: long side and end of the box, per branch
over the ego headings HEADINGS and the origins ORIGINS; the obstacle heading is the family's own and is rounded on its own.

PACKING.  A slot is the +delta and the -delta version of one configuration; both share the ego poses.  Dynamic slots of one origin are
dealt round-robin to TRAJS lattice cells 200 m apart (cell 0: the origin itself).  dynamic_batch: a cell is a trajectory, its cases
follow one another (+ in front of -), case q takes the poses 2 q and 2 q + 1 (a pose given twice; the two poses of a swept case) and
its obstacle is present at time index 2 q only: every other row is NaN, so the odd poses and segments see nothing.  case_batch: the
same scene, one trajectory per case (every first hit is a case's verdict).  member_batch (ensemble): one trajectory per slot, its +
version in member 0 and its - version in member 1 at the same time index.  Static cases stand one per cell of such a lattice, at
most LDS_ROWS to a scene.  Every foreign shape is more than 50 m away (asserted).

usage: python tests/_contact.py [out_file]      writes profiles/accuracy_contact.txt (on a GPU box: with the device's verdicts per path)"""
import dataclasses
import functools
import math
import os
import sys

import numpy as np

if __name__ == "__main__":   # (as a script: the paths tests/conftest.py sets up for the suite)
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "commonroad-reactive-planner_amd"), os.path.join(_repo, "tests")]

import _dd as dd
from _dd import DD
from _xref import HAVE_LONGDOUBLE, SKIP_REASON   # noqa: F401  (what the tests skip with)

from commonroad_rp_amd._capi import make_params
from commonroad_rp_amd.collision import ObstacleTables

LD = np.longdouble
U = 2.0 ** -53
BAND = 8.0                   # B = BAND u scale
DECIDED = 8.0                # every case: |g| >= DECIDED B
HL, HW, WB = 2.254, 0.805, 1.4227
EGO_R = math.hypot(HL, HW)
BETA = math.atan2(HW, HL)    # the ego's diagonal against its heading
HEADINGS = (0.0, 0.5 * math.pi, math.pi, -math.pi, 0.25 * math.pi, 0.3, 2.0, -2.7, 7.0)
ORIGINS = ((0.0, 0.0), (1e3, -7e2), (1e5, -7e4), (3e6, -2.1e6))
DISPLACEMENTS = ("64B", "65536B", "1e-6")
SPACING = 200.0              # metres between the cells of a lattice
FOREIGN = 50.0               # metres every foreign shape keeps from a case
TRAJS, POSES = 65, 63        # the ragged batch of the dynamic cases of one origin
LDS_ROWS = 128               # static shapes to a scene (CK_LDS_ROWS; tests/test_contact_abi.py checks the number against the source)
BRANCH_MARGIN = 1e-3
FAR = 5.0e4                  # metres: where a pose that must see nothing stands


def params(n=2, time_step0=0, factor=1):
    return make_params(dt=0.1, N=n - 1, factor=factor, time_step0=time_step0, low_vel_mode=False, lon_mode=0, constraint_mask=0, flags=0,
                       x0_lon=[0, 0, 0], x0_lat=[0, 0, 0], x0_orientation=0.0, wheelbase=2.5789, wb_rear_axle=WB, length=2 * HL,
                       width=2 * HW, a_max=11.5, v_switch=7.319, delta_max=1.066, v_delta_max=0.4)


# ---- the reference: double-word geometry, vectorised over cases ------------------------------------------------------------------
def _d(a):
    """doubles (or longdoubles) as double-word numbers, exactly"""
    return a if isinstance(a, DD) else DD(np.asarray(a).astype(LD))


def _max(a, b):
    return dd.where(a > b, a, b)


def _min(a, b):
    return dd.where(a < b, a, b)


@dataclasses.dataclass
class Box:
    cx: DD
    cy: DD
    ux: DD
    uy: DD
    hl: DD
    hw: DD

    def take(self, k):
        return Box(*(getattr(self, f.name)[k] for f in dataclasses.fields(self)))


def ego_box(x, y, th, hl=HL, hw=HW, wb=WB):
    s, c = dd.sincos(_d(th))
    n = np.shape(x)
    return Box(_d(x) + c * wb, _d(y) + s * wb, c, s, _d(np.full(n, hl)), _d(np.full(n, hw)))


def rect_box(rows):
    """rows [N, >= 5] of doubles: cx, cy, theta, hl, hw"""
    s, c = dd.sincos(_d(rows[:, 2]))
    return Box(_d(rows[:, 0]), _d(rows[:, 1]), c, s, _d(rows[:, 3]), _d(rows[:, 4]))


def merge(a: Box, b: Box):
    """The rectangle around a and b; (box, centre distance - lim, heading dot product) -- the two branch switches."""
    dx, dy = b.cx - a.cx, b.cy - a.cy
    lim = (_max(a.hl, a.hw) + _max(b.hl, b.hw)).scaled(2.0)
    dist = dd.sqrt(dx * dx + dy * dy)
    far = dist > lim
    dot = a.ux * b.ux + a.uy * b.uy
    sgn = np.where(dot < 0.0, LD(-1.0), LD(1.0))
    nx, ny = dd.where(far, dx, a.ux + b.ux * sgn), dd.where(far, dy, a.uy + b.uy * sgn)
    nrm = dd.sqrt(nx * nx + ny * ny)
    nx, ny = nx / nrm, ny / nrm
    mx, my = -ny, nx
    lo, hi = [], []
    for ex, ey in ((nx, ny), (mx, my)):
        ea = a.hl * abs(a.ux * ex + a.uy * ey) + a.hw * abs(a.uy * ex - a.ux * ey)
        eb = b.hl * abs(b.ux * ex + b.uy * ey) + b.hw * abs(b.uy * ex - b.ux * ey)
        pb = dx * ex + dy * ey
        lo.append(_min(-ea, pb - eb))
        hi.append(_max(ea, pb + eb))
    c0, c1 = (lo[0] + hi[0]).scaled(0.5), (lo[1] + hi[1]).scaled(0.5)
    box = Box(a.cx + (c0 * nx + c1 * mx), a.cy + (c0 * ny + c1 * my), nx, ny, (hi[0] - lo[0]).scaled(0.5), (hi[1] - lo[1]).scaled(0.5))
    return box, (dist - lim).ld(), dot.ld()


def gap_rect(e: Box, o: Box):
    tx, ty = o.cx - e.cx, o.cy - e.cy
    g = None
    for nx, ny in ((e.ux, e.uy), (-e.uy, e.ux), (o.ux, o.uy), (-o.uy, o.ux)):
        re = e.hl * abs(e.ux * nx + e.uy * ny) + e.hw * abs(e.ux * ny - e.uy * nx)
        ro = o.hl * abs(o.ux * nx + o.uy * ny) + o.hw * abs(o.ux * ny - o.uy * nx)
        sep = abs(tx * nx + ty * ny) - (re + ro)
        g = sep if g is None else _max(g, sep)
    return g


def _local(e: Box, px, py):
    qx, qy = px - e.cx, py - e.cy
    return qx * e.ux + qy * e.uy, qy * e.ux - qx * e.uy


def gap_tri(e: Box, vx, vy):
    """vx, vy: three DD each"""
    loc = [_local(e, vx[k], vy[k]) for k in range(3)]
    lx, ly = [p[0] for p in loc], [p[1] for p in loc]

    def spread(p, r):
        lo, hi = _min(_min(p[0], p[1]), p[2]), _max(_max(p[0], p[1]), p[2])
        return _max(lo - r, -hi - r)
    g = _max(spread(lx, e.hl), spread(ly, e.hw))
    for k in range(3):
        k2 = (k + 1) % 3
        ex, ey = lx[k2] - lx[k], ly[k2] - ly[k]
        ln = dd.sqrt(ex * ex + ey * ey)
        ok = ln > 0.0
        ln = dd.where(ok, ln, 1.0)
        nx, ny = -ey / ln, ex / ln
        sep = spread([lx[j] * nx + ly[j] * ny for j in range(3)], e.hl * abs(nx) + e.hw * abs(ny))
        g = dd.where(ok, _max(g, sep), g)
    return g


def gap_circ(e: Box, cx, cy, r):
    lx, ly = _local(e, cx, cy)
    ax, ay = abs(lx) - e.hl, abs(ly) - e.hw
    outside = (ax > 0.0) | (ay > 0.0)
    dx, dy = _max(ax, 0.0), _max(ay, 0.0)
    return dd.where(outside, dd.sqrt(dx * dx + dy * dy), _max(ax, ay)) - r


def corners(b: Box):
    out = []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        out.append((b.cx + (b.hl * b.ux) * sx - (b.hw * b.uy) * sy, b.cy + (b.hl * b.uy) * sx + (b.hw * b.ux) * sy))
    return out


def _point_segment(px, py, ax, ay, bx, by):
    ex, ey, qx, qy = bx - ax, by - ay, px - ax, py - ay
    den = ex * ex + ey * ey
    ok = den > 0.0
    t = (qx * ex + qy * ey) / dd.where(ok, den, 1.0)
    t = dd.where(ok, _min(_max(t, 0.0), 1.0), 0.0)
    rx, ry = qx - t * ex, qy - t * ey
    return dd.sqrt(rx * rx + ry * ry)


def polygon_distance(P, Q):
    """P, Q: lists of (x, y) DD vertices: the minimum vertex-to-segment distance, both ways (the distance of disjoint polygons)"""
    best = None
    for A, B in ((P, Q), (Q, P)):
        for px, py in A:
            for k in range(len(B)):
                d = _point_segment(px, py, *B[k], *B[(k + 1) % len(B)])
                best = d if best is None else _min(best, d)
    return best


# ---- the families ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Variant:
    """An obstacle in the frame of the ego rectangle (swept: of the merged box): the obstacle's reference point is
    base + t (cos dir, sin dir); contact is found by bisection over t in `bracket` (overlapping at its left end)."""
    name: str
    family: str
    kind: str                 # rect | tri | circ
    shape: tuple              # rect: (heading, hl, hw) | tri: three (x, y) around the reference point | circ: (r,)
    base: tuple = (0.0, 0.0)
    dir: float = 0.0
    bracket: tuple = (0.0, 300.0)
    full: bool = False        # all three displacements at every heading and origin (else one of them, in rotation)
    fixed: bool = False       # containment: no contact, the obstacle stays at `base`
    second: tuple = None      # swept: the second pose in the frame of the first (dx, dy, dtheta)


def _rect(name, family, heading, hl, hw, **kw):
    return Variant(name, family, "rect", (heading, hl, hw), **kw)


def _corner(name, direction, hl, hw):
    return _rect(name, "c", direction - math.atan2(hw, hl), hl, hw, dir=direction, full=True)


_P4, _P2 = 0.25 * math.pi, 0.5 * math.pi
_E5 = 50.0 / math.sqrt(2.0)
VARIANTS = (
    _rect("a_front", "a", 0.0, 1.0, 0.5, base=(0.0, 0.4), dir=0.0),
    _rect("a_left_upright", "a", _P2, 1.0, 0.5, base=(-0.7, 0.0), dir=_P2),
    _rect("a_rear_reversed", "a", math.pi, 1.0, 0.5, base=(0.0, -0.3), dir=math.pi),
    _rect("a_segment_parallel", "a", 0.0, 1.5, 0.0, base=(0.5, 0.0), dir=-_P2),
    _rect("a_segment_across", "a", _P2, 1.5, 0.0, base=(0.0, 0.2), dir=0.0),
    _rect("b_its_corner", "b", 0.5, 1.2, 0.6, base=(0.0, 0.2), dir=0.0),
    _rect("b_ego_corner", "b", 0.6, 1.5, 2.5, dir=0.6),
    _corner("c_front_left", BETA, 1.0, 0.5),
    _corner("c_rear_left_square", math.pi - BETA, 0.7, 0.7),
    _corner("c_front_right_thin", -BETA, 3.0, 0.2),
    _rect("d_square", "d", _P4, 1.0, 1.0, base=(HL, HW), dir=_P4, bracket=(0.0, 100.0), full=True),
    _rect("d_rear_oblong", "d", 3 * _P4, 1.3, 0.9, base=(-HL, HW), dir=3 * _P4, bracket=(0.0, 100.0), full=True),
    _rect("e_inside_ego", "e", 0.7, 0.3, 0.2, base=(0.5, 0.1), fixed=True),
    _rect("e_ego_inside", "e", 0.3, 8.0, 6.0, base=(1.0, -0.5), fixed=True),
    _rect("e_ego_in_a_far_corner", "e", 0.3, 40.0, 30.0, base=(30.0, 20.0), fixed=True),
    _rect("f_end_on_diagonal", "f", BETA, 40.0, 0.05, dir=BETA, full=True),
    _rect("f_end_on_diagonal_hw0", "f", BETA, 40.0, 0.0, dir=BETA, full=True),
    _rect("f_end_beside", "f", 0.0, 40.0, 0.05, base=(HL + 39.5, 0.0), dir=_P2),
    _rect("f_mid_across_hw0", "f", _P2, 40.0, 0.0, base=(0.0, 5.0), dir=0.0),
    _rect("f_mid_oblique", "f", 0.9, 40.0, 0.05, base=(7.0 * math.cos(0.9), 7.0 * math.sin(0.9)), dir=0.9 + _P2),
    _rect("f_mid_oblique_hw0", "f", 0.9, 40.0, 0.0, base=(7.0 * math.cos(0.9), 7.0 * math.sin(0.9)), dir=0.9 + _P2),
    _rect("f_far_end_normal_on_diagonal", "f", BETA - _P2, 40.0, 0.05, base=(39.9 * math.cos(BETA - _P2), 39.9 * math.sin(BETA - _P2)),
          dir=BETA, full=True),
    Variant("g_vertex_on_edge", "g", "tri", ((0.0, 0.0), (2.0, 1.0), (2.0, -1.0)), base=(0.0, 0.2)),
    Variant("g_edge_through_corner", "g", "tri", ((1.0, -1.0), (-1.0, 1.0), (2.0, 2.25)), base=(HL, HW), dir=_P4, bracket=(-0.5, 100.0)),
    Variant("g_collinear_end", "g", "tri", ((0.0, 0.0), (1.0, 0.5), (3.0, 1.5)), base=(0.0, -0.3)),
    Variant("g_collinear_through_corner", "g", "tri", ((1.0, -1.0), (-1.0, 1.0), (0.25, -0.25)), base=(HL, HW), dir=_P4, bracket=(-0.5, 100.0)),
    Variant("g_vertex_on_edge_clockwise", "g", "tri", ((0.0, 0.0), (2.0, -1.0), (2.0, 1.0)), base=(0.0, 0.2)),
    Variant("g_edge_through_corner_clockwise", "g", "tri", ((2.0, 2.25), (-1.0, 1.0), (1.0, -1.0)), base=(HL, HW), dir=_P4, bracket=(-0.5, 100.0)),
    Variant("g_100m_edge", "g", "tri", ((_E5, -_E5), (-_E5, _E5), (30.0, 30.0)), base=(HL, HW), dir=_P4, bracket=(-0.5, 100.0)),
    Variant("h_on_edge", "h", "circ", (1.0,), base=(0.5, 0.0), dir=_P2),
    Variant("h_on_corner", "h", "circ", (5.0,), base=(HL, HW), dir=0.9, bracket=(-0.3, 100.0)),
    Variant("h_point_on_edge", "h", "circ", (0.0,), base=(0.0, 0.3)),
    Variant("h_point_on_corner", "h", "circ", (0.0,), base=(HL, -HW), dir=-0.5, bracket=(-0.3, 100.0)),
    _rect("i_bisector_side", "i", 0.4, 1.0, 0.5, base=(0.3, 0.0), dir=_P2, second=(1.2, 0.15, 0.2)),
    _rect("i_bisector_end", "i", 0.0, 1.0, 0.5, base=(0.0, 0.2), dir=0.0, second=(1.2, 0.15, 0.2)),
    _rect("i_reversed_side", "i", 0.4, 1.0, 0.5, base=(0.3, 0.0), dir=_P2, second=(0.8, 0.1, 2.9)),
    _rect("i_reversed_end", "i", 0.0, 1.0, 0.5, base=(0.0, 0.2), dir=0.0, second=(0.8, 0.1, 2.9)),
    _rect("i_centre_line_side", "i", 0.4, 1.0, 0.5, base=(0.3, 0.0), dir=_P2, second=(12.0, 3.0, 0.3)),
    _rect("i_centre_line_end", "i", 0.0, 1.0, 0.5, base=(0.0, 0.2), dir=0.0, second=(12.0, 3.0, 0.3)),
)
FAMILIES = tuple(sorted({v.family for v in VARIANTS}))


# ---- the table -------------------------------------------------------------------------------------------------------------------
class Table:
    """Arrays over the cases, read-only.  vid, oi, hi, dk (displacement kind, -1: none), sign (+1 apart, -1 overlapping, 0: containment),
    static, slot (the +- pair), scene (dynamic: the origin; static: the scene), traj, pos (dynamic: slot within the trajectory; static: cell),
    a, b [N, 3] (the ego's rear-axle poses; a == b but for family i), row [N, 6] (NaN-padded obstacle row), g (the case's gap: of the ego
    rectangle, family i: of the merged box; g + g_lo: before rounding to longdouble), g_pose (ego rectangle of pose a), g_pose_b (of pose b), dist (distance of that rectangle, where g_pose > 0),
    B, B_pose, hit, hit_pose, kind, family, name."""

    def __len__(self):
        return len(self.vid)

    def select(self, **kw):
        m = np.ones(len(self), bool)
        for k, v in kw.items():
            m &= np.isin(getattr(self, k), v)
        return np.flatnonzero(m)


def _slots():
    """(vid, oi, hi, dk, static) of every slot, in table order: by origin, then static after dynamic, then variant, heading"""
    out = []
    for oi in range(len(ORIGINS)):
        for static in (False, True):
            for vi, v in enumerate(VARIANTS):
                for hi in range(len(HEADINGS)):
                    if v.kind == "rect" and static and hi != (vi + oi) % len(HEADINGS):
                        continue     # rectangles are dynamic in the main; one static copy per variant and origin
                    if v.kind != "rect" and not static:
                        continue     # triangles and circles are static shapes
                    rot = (vi + hi + oi) % 3
                    for dk in ((-1,) if v.fixed else (0, 1, 2) if (v.full and not static) else (rot,)):
                        out.append((vi, oi, hi, dk, static))
    return out


def _lattice(k, per_row):
    return SPACING * (k % per_row), SPACING * (k // per_row)


def _rot(c, s, x, y):
    return c * x - s * y, s * x + c * y


def _obstacle_at(T, idx, frame, t):
    """Obstacle of the cases idx (all of one kind) with its reference point at parameter t (longdouble): rectangle -> (cx, cy),
    triangle -> (vx [3], vy [3]), circle -> (cx, cy), all longdouble."""
    fx, fy, fc, fs = (f[idx] for f in frame)
    bx, by = T._base[idx, 0] + t * np.cos(T._dir[idx].astype(LD)), T._base[idx, 1] + t * np.sin(T._dir[idx].astype(LD))
    px, py = _rot(fc, fs, bx, by)
    px, py = fx + px, fy + py
    if T.kind[idx[0]] != "tri":
        return px, py
    vx, vy = [], []
    for k in range(3):
        ox, oy = _rot(fc, fs, T._tri[idx, k, 0].astype(LD), T._tri[idx, k, 1].astype(LD))
        vx.append(px + ox)
        vy.append(py + oy)
    return vx, vy


def _gap_of(T, idx, boxes: Box, obstacle, axes):
    """gap of the boxes (already taken at idx) to the obstacle (longdouble or double coordinates)"""
    kind = T.kind[idx[0]]
    if kind == "rect":
        return gap_rect(boxes, Box(_d(obstacle[0]), _d(obstacle[1]), axes[0], axes[1], _d(T._shape[idx, 1]), _d(T._shape[idx, 2])))
    if kind == "tri":
        return gap_tri(boxes, [_d(v) for v in obstacle[0]], [_d(v) for v in obstacle[1]])
    return gap_circ(boxes, _d(obstacle[0]), _d(obstacle[1]), _d(T._shape[idx, 0]))


def _radius(T, idx, row):
    kind = T.kind[idx[0]]
    if kind == "rect":
        return np.hypot(row[:, 3], row[:, 4]), row[:, 0], row[:, 1]
    if kind == "circ":
        return row[:, 2], row[:, 0], row[:, 1]
    cx, cy = row[:, 0:6:2].mean(1), row[:, 1:6:2].mean(1)
    return np.hypot(row[:, 0:6:2] - cx[:, None], row[:, 1:6:2] - cy[:, None]).max(1), cx, cy


def _band(box: Box, row_r, row_cx, row_cy):
    ecx, ecy = np.asarray(box.cx.ld(), float), np.asarray(box.cy.ld(), float)
    er = np.hypot(np.asarray(box.hl.ld(), float), np.asarray(box.hw.ld(), float))
    scale = np.abs(ecx) + np.abs(ecy) + er + row_r + np.hypot(row_cx - ecx, row_cy - ecy)
    return BAND * U * scale


def _bisect(T, idx, Ei, frame, axes, lo, hi, mov):
    """the parameter of the contact (the first one apart, to a longdouble ulp) of the cases idx between lo (overlapping) and hi"""
    a, b = lo.copy(), hi.copy()
    ga = _gap_of(T, idx, Ei, _obstacle_at(T, idx, frame, a), axes)
    gb = _gap_of(T, idx, Ei, _obstacle_at(T, idx, frame, b), axes)
    assert np.all((ga <= 0.0)[mov]) and np.all((gb > 0.0)[mov]), (T.kind[idx[0]], "a bracket does not straddle the contact")
    for _ in range(80):
        mid = 0.5 * (a + b)
        apart = _gap_of(T, idx, Ei, _obstacle_at(T, idx, frame, mid), axes) > 0.0
        a, b = np.where(apart, a, mid), np.where(apart, mid, b)
    return b


def _build(slots, ladder=None):
    """The table of the given slots.  ladder: None -> the +- displacement of each slot's kind; else a list of multiples k: the cases
    are the contact displaced by +- k u scale (the measurement of the double predicate's own error; no conditions asserted)."""
    T = Table()
    signs = (1, -1)
    rec = []
    for si, (vi, oi, hi, dk, static) in enumerate(slots):
        if VARIANTS[vi].fixed:
            rec.append((vi, oi, hi, dk, static, si, 0, 0.0))
        elif ladder is None:
            rec += [(vi, oi, hi, dk, static, si, sg, 0.0) for sg in signs]
        else:
            rec += [(vi, oi, hi, dk, static, si, sg, float(k)) for k in ladder for sg in signs]
    N = len(rec)
    T.vid, T.oi, T.hi, T.dk = (np.array([r[q] for r in rec], dtype=np.int32) for q in range(4))
    T.static = np.array([r[4] for r in rec], dtype=bool)
    T.slot = np.array([r[5] for r in rec], dtype=np.int32)
    T.sign = np.array([r[6] for r in rec], dtype=np.int32)
    T._k = np.array([r[7] for r in rec])
    T.kind = np.array([VARIANTS[v].kind for v in T.vid])
    T.family = np.array([VARIANTS[v].family for v in T.vid])
    T.name = np.array([VARIANTS[v].name for v in T.vid])
    T.swept = np.array([VARIANTS[v].second is not None for v in T.vid])

    # -- the layout: scene, trajectory, position, and from them the ego's place
    T.scene, T.traj, T.pos = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    cell = np.zeros((N, 2))
    slot_cases = {}
    for i in range(N):
        slot_cases.setdefault(int(T.slot[i]), []).append(i)
    dyn_count, stat_count, scene_of = {}, {}, {}
    for si, cs in slot_cases.items():
        vi, oi, hi, dk, static = slots[si]
        if not static:
            n = dyn_count.get(oi, 0)
            dyn_count[oi] = n + 1
            k, p = n % TRAJS, n // TRAJS
            assert ladder is not None or 2 * p + 2 <= POSES, "more dynamic slots than the ragged batch of one origin holds"
            for i in cs:
                T.scene[i], T.traj[i], T.pos[i] = oi, k, p
                cell[i] = _lattice(k, 9)
        else:
            for i in cs:       # a static case has a place of its own
                n = stat_count.get(oi, 0)
                stat_count[oi] = n + 1
                key = (oi, n // LDS_ROWS)
                scene_of.setdefault(key, len(scene_of))
                T.scene[i], T.traj[i], T.pos[i] = scene_of[key], 0, n % LDS_ROWS
                cell[i] = _lattice(n % LDS_ROWS, 12)
    T.n_static_scenes = len(scene_of)
    org = np.array(ORIGINS)[T.oi]
    tha = np.array(HEADINGS)[T.hi]
    T.a = np.stack((org[:, 0] + cell[:, 0], org[:, 1] + cell[:, 1], tha), 1)
    sec = np.array([VARIANTS[v].second or (0.0, 0.0, 0.0) for v in T.vid])
    bx, by = _rot(np.cos(tha), np.sin(tha), sec[:, 0], sec[:, 1])
    T.b = np.stack((T.a[:, 0] + bx, T.a[:, 1] + by, tha + sec[:, 2]), 1)

    # -- per-case variant data
    T._base = np.array([VARIANTS[v].base for v in T.vid]).astype(LD)
    T._dir = np.array([VARIANTS[v].dir for v in T.vid])
    T._shape = np.array([(tuple(VARIANTS[v].shape) + (0.0, 0.0, 0.0))[:3] if VARIANTS[v].kind != "tri" else (0.0, 0.0, 0.0) for v in T.vid])
    T._tri = np.array([VARIANTS[v].shape if VARIANTS[v].kind == "tri" else ((0.0, 0.0),) * 3 for v in T.vid])
    lo = np.array([VARIANTS[v].bracket[0] for v in T.vid]).astype(LD)
    hi = np.array([VARIANTS[v].bracket[1] for v in T.vid]).astype(LD)
    fixed = np.array([VARIANTS[v].fixed for v in T.vid])

    # -- ego rectangles, merged boxes, the frame the variant is stated in
    A, Bx = ego_box(T.a[:, 0], T.a[:, 1], T.a[:, 2]), ego_box(T.b[:, 0], T.b[:, 1], T.b[:, 2])
    M, d_lim, dot = merge(A, Bx)
    sw = T.swept
    assert np.all(np.abs(d_lim[sw]) >= BRANCH_MARGIN) and np.all(np.abs(dot[sw]) >= BRANCH_MARGIN), "a swept case next to a branch switch"
    T.branch = np.where(d_lim > 0, 2, np.where(dot < 0, 1, 0))     # 0 bisector | 1 bisector, reversed | 2 centre line
    pick = lambda f: dd.where(sw, getattr(M, f), getattr(A, f))   # noqa: E731   (a == b: the merged box IS the rectangle)
    E = Box(*(pick(f.name) for f in dataclasses.fields(Box)))
    frame = (E.cx.ld(), E.cy.ld(), E.ux.ld(), E.uy.ld())
    heading = np.arctan2(frame[3], frame[2])
    phi = np.asarray(heading + T._shape[:, 0].astype(LD), dtype=np.float64)       # the obstacle's heading: a double of its own
    os_, oc_ = dd.sincos(_d(phi))

    # -- contact by bisection, the displacement, the rounded obstacle
    T.row = np.full((N, 6), np.nan)
    for kind in ("rect", "tri", "circ"):
        idx = np.flatnonzero(T.kind == kind)
        if not len(idx):
            continue
        Ei, axes = E.take(idx), (oc_[idx], os_[idx])
        mov = ~fixed[idx]
        b = _bisect(T, idx, Ei, frame, axes, lo[idx], hi[idx], mov)
        t0 = np.where(mov, b, LD(0.0))
        # B at the contact (the final one, from the rounded doubles, differs from it by rounding only)
        ob = _obstacle_at(T, idx, frame, t0)
        row0 = _row_of(T, idx, ob, phi)
        B0 = _band(Ei, *_radius(T, idx, row0))
        if ladder is None:
            mag = np.where(T.dk[idx] == 0, 64.0 * B0, np.where(T.dk[idx] == 1, 65536.0 * B0, 1e-6))
        else:
            mag = T._k[idx] * U * (B0 / (BAND * U))
        t = t0 + np.where(mov, T.sign[idx] * mag, 0.0).astype(LD)
        T.row[idx] = _row_of(T, idx, _obstacle_at(T, idx, frame, t), phi)

    # -- the verdicts, from the doubles alone
    T.g, T.g_lo, T.g_pose, T.dist = np.zeros(N, LD), np.zeros(N, LD), np.zeros(N, LD), np.full(N, np.inf, LD)
    T.g_pose_b, T.B, T.B_pose, T.B_pose_b = np.zeros(N, LD), np.zeros(N), np.zeros(N), np.zeros(N)
    for kind in ("rect", "tri", "circ"):
        idx = np.flatnonzero(T.kind == kind)
        if not len(idx):
            continue
        row = T.row[idx]
        Ei, Ai = E.take(idx), A.take(idx)
        if kind == "rect":
            ob = rect_box(row)
            gd = gap_rect(Ei, ob)
            T.g_pose[idx], T.g_pose_b[idx] = gap_rect(Ai, ob).ld(), gap_rect(Bx.take(idx), ob).ld()
            T.dist[idx] = polygon_distance(corners(Ai), corners(ob)).ld()
        elif kind == "tri":
            vx, vy = [_d(row[:, 2 * k]) for k in range(3)], [_d(row[:, 2 * k + 1]) for k in range(3)]
            gd = gap_tri(Ai, vx, vy)
            T.g_pose[idx] = T.g_pose_b[idx] = gd.ld()
            T.dist[idx] = polygon_distance(corners(Ai), list(zip(vx, vy))).ld()
        else:
            gd = gap_circ(Ai, _d(row[:, 0]), _d(row[:, 1]), _d(row[:, 2]))
            T.g_pose[idx] = T.g_pose_b[idx] = T.dist[idx] = gd.ld()
        T.g[idx] = gd.ld()
        T.g_lo[idx] = (gd - DD(T.g[idx])).ld()      # g + g_lo: the double-word gap itself
        rad = _radius(T, idx, row)
        T.B[idx], T.B_pose[idx], T.B_pose_b[idx] = _band(Ei, *rad), _band(Ai, *rad), _band(Bx.take(idx), *rad)
    T.hit, T.hit_pose, T.hit_pose_b = T.g <= 0, T.g_pose <= 0, T.g_pose_b <= 0
    T.dist = np.where(T.hit_pose, LD(0.0), T.dist)
    T.ladder = ladder is not None
    if ladder is None:
        _assert_conditions(T)
    for v in vars(T).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return T


def _row_of(T, idx, ob, phi):
    kind = T.kind[idx[0]]
    row = np.full((len(idx), 6), np.nan)
    if kind == "rect":
        row[:, 0], row[:, 1], row[:, 2], row[:, 3], row[:, 4] = ob[0], ob[1], phi[idx], T._shape[idx, 1], T._shape[idx, 2]
    elif kind == "circ":
        row[:, 0], row[:, 1], row[:, 2] = ob[0], ob[1], T._shape[idx, 0]
    else:
        for k in range(3):
            row[:, 2 * k], row[:, 2 * k + 1] = ob[0][k], ob[1][k]
    return row


def _assert_conditions(T):
    """Every case decided with the intended sign; every foreign shape more than FOREIGN away."""
    g, gp = np.asarray(T.g, float), np.asarray(T.g_pose, float)
    bad = np.flatnonzero(np.abs(g) < DECIDED * T.B)
    assert not len(bad), ("undecided", [(T.name[i], int(T.oi[i]), int(T.hi[i]), int(T.dk[i]), g[i] / T.B[i]) for i in bad[:8]])
    want = np.where(T.sign == 0, -1, T.sign)
    bad = np.flatnonzero(np.sign(g) != want)
    assert not len(bad), ("sign", [(T.name[i], int(T.oi[i]), int(T.hi[i]), g[i]) for i in bad[:8]])
    bad = np.flatnonzero((np.abs(gp) < DECIDED * T.B_pose) | (np.abs(np.asarray(T.g_pose_b, float)) < DECIDED * T.B_pose_b))
    # (family i: the rectangles of the two poses are asked about as well)
    assert not len(bad), ("pose undecided", [(T.name[i], int(T.oi[i]), int(T.hi[i]), gp[i] / T.B_pose[i]) for i in bad[:8]])
    rad, cx, cy = np.zeros(len(T)), np.zeros(len(T)), np.zeros(len(T))
    for kind in ("rect", "tri", "circ"):
        idx = np.flatnonzero(T.kind == kind)
        rad[idx], cx[idx], cy[idx] = _radius(T, idx, T.row[idx])
    # a foreign shape: static -- every other shape of the scene; dynamic -- the shapes of the origin's other trajectories (those of the
    # case's own trajectory are present at other time indices only)
    for static in (False, True):
        for sc in np.unique(T.scene[T.static == static]):
            sub = np.flatnonzero((T.static == static) & (T.scene == sc))
            foreign = ~np.eye(len(sub), dtype=bool) if static else T.traj[sub, None] != T.traj[None, sub]
            for pose in (T.a, T.b):
                d = np.hypot(pose[sub, None, 0] - cx[None, sub], pose[sub, None, 1] - cy[None, sub]) - rad[None, sub] - (EGO_R + WB)
                assert np.all(d[foreign] > FOREIGN), "a foreign shape within reach"


@functools.lru_cache(maxsize=None)
def table() -> Table:
    return _build(_slots())


LADDER = (1, 2, 4, 8, 16, 32, 64, 1 << 10, 1 << 16, 1 << 20)


def ladder_table() -> Table:
    """The contacts of one heading in three (in rotation) displaced by +- k u scale, k in LADDER: what the double predicate's own error
    is measured on."""
    seen = sorted({(vi, oi, hi, 0, static) for vi, oi, hi, _, static in _slots() if not VARIANTS[vi].fixed and hi % 3 == (vi + oi) % 3},
                  key=lambda s: (s[1], s[4], s[0], s[2]))
    return _build(seen, ladder=LADDER)


# ---- packing ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Batch:
    """One call: poses [K, n], lengths [K], the obstacle tables, and where each case sits: case [K, n] (index into the table or -1) for
    the pose verdict, seg_case [K, n] for the segment that starts at the pose."""
    x: np.ndarray
    y: np.ndarray
    th: np.ndarray
    lengths: np.ndarray
    obstacles: ObstacleTables
    case: np.ndarray
    seg_case: np.ndarray
    members: np.ndarray = None       # [2, n_dyn, n_steps, 5]: the + and the - version of every slot (dynamic batches)
    case_b: np.ndarray = None        # [K, n]: where a pose is a case's SECOND pose and sees its obstacle (static cases), else -1

    def expected(self, T):
        """(pose_hits [K, n], first_pose_hit [K], first_segment_hit [K]) of the reference"""
        K, n = self.case.shape
        ph = np.where(self.case >= 0, T.hit_pose[np.maximum(self.case, 0)], False)
        if self.case_b is not None:
            ph = ph | np.where(self.case_b >= 0, T.hit_pose_b[np.maximum(self.case_b, 0)], False)
        sh = np.where(self.seg_case >= 0, T.hit[np.maximum(self.seg_case, 0)], False)
        first = lambda h: np.where(h.any(1), h.argmax(1), -1).astype(np.int32)   # noqa: E731
        return ph, first(ph), first(sh)


def _tables(T, cases, n_steps=0, steps=None, pad_static=0):
    """ObstacleTables of the given cases: static ones in table order (rectangles, triangles, circles: ids in that order), dynamic ones one
    obstacle each, present at its step only.  pad_static: far rectangles added BEHIND the rectangles of the cases."""
    st = [i for i in cases if T.static[i]]
    sobb = [T.row[i, :5] for i in st if T.kind[i] == "rect"]
    tri = [T.row[i, :6] for i in st if T.kind[i] == "tri"]
    circ = [T.row[i, :3] for i in st if T.kind[i] == "circ"]
    for q in range(pad_static):
        sobb.append([-FAR - 10.0 * q, FAR, 0.3, 2.0, 1.0])
    dyn_cases = [i for i in cases if not T.static[i]]
    dyn = np.full((len(dyn_cases), n_steps, 5), np.nan)
    for j, i in enumerate(dyn_cases):
        dyn[j, steps[i]] = T.row[i, :5]
    return ObstacleTables(static_obb=sobb or None, static_tri=tri or None, static_circ=circ or None, dyn_obb=dyn, dyn_t0=0)


def static_ids(T, cases):
    """obstacle id (rp_clearance.h: static rectangles, triangles, circles, then dynamic obstacles) of every static case of a scene"""
    st = [i for i in cases if T.static[i]]
    order = [i for k in ("rect", "tri", "circ") for i in st if T.kind[i] == k]
    return {i: q for q, i in enumerate(order)}


def dynamic_batch(T, origin):
    """The dynamic cases of one origin as TRAJS x POSES ragged trajectories: the cases of a lattice cell one after the other, a pose pair
    each, the + version of a slot in front of its - version.  Every pose flag is a case's verdict; first_pose_hit and
    first_segment_hit are those of the trajectory's first overlapping case alone (case_batch shows every case's)."""
    idx = T.select(static=False, scene=origin)
    K, n = int(T.traj[idx].max()) + 1, POSES
    x, y, th = (np.zeros((K, n)) for _ in range(3))
    case, seg = np.full((K, n), -1), np.full((K, n), -1)
    lengths = np.zeros(K, np.int32)
    steps = {}
    order = {}
    for i in idx:
        order.setdefault(int(T.traj[i]), []).append(i)
    for k, cs in order.items():
        cs.sort(key=lambda i: (T.pos[i], -T.sign[i]))
        assert 2 * len(cs) <= n - 1
        for q, i in enumerate(cs):
            x[k, 2 * q], y[k, 2 * q], th[k, 2 * q] = T.a[i]
            x[k, 2 * q + 1], y[k, 2 * q + 1], th[k, 2 * q + 1] = T.b[i]
            case[k, 2 * q], seg[k, 2 * q], steps[i] = i, i, 2 * q
        L = 2 * len(cs) + (k % 2)       # ragged; an odd length ends on one more copy of the last pose
        if k % 2:
            x[k, L - 1], y[k, L - 1], th[k, L - 1] = x[k, L - 2], y[k, L - 2], th[k, L - 2]
        lengths[k] = L
    return Batch(x, y, th, lengths, _tables(T, list(idx), n_steps=n, steps=steps), case, seg)


def case_batch(T, origin):
    """The same scene as dynamic_batch(T, origin) -- its obstacle table, every case at its time index -- with ONE TRAJECTORY PER CASE:
    the case's pose pair at that time index behind poses that stand FAR away, the trajectory ends with the pair.  first_pose_hit and
    first_segment_hit of a trajectory are then the verdicts of its case: the segment verdict of every dynamic case is seen."""
    b = dynamic_batch(T, origin)
    ks, qs = np.nonzero(b.case >= 0)
    K, n = len(ks), int(qs.max()) + 2
    x, y, th = np.full((K, n), ORIGINS[origin][0] - FAR), np.full((K, n), ORIGINS[origin][1] - FAR), np.zeros((K, n))
    case = np.full((K, n), -1)
    r = np.arange(K)
    for d in (0, 1):
        x[r, qs + d], y[r, qs + d], th[r, qs + d] = b.x[ks, qs + d], b.y[ks, qs + d], b.th[ks, qs + d]
    case[r, qs] = b.case[ks, qs]
    return Batch(x, y, th, (qs + 2).astype(np.int32), b.obstacles, case, case.copy())


def single_batch(T, n=130):
    """1 x n: every m-th dynamic case of the whole table, a pose given twice each (family i: its two poses)"""
    idx = T.select(static=False)
    take = idx[np.unique(np.linspace(0, len(idx) - 1, n // 2).astype(int))]
    x, y, th = (np.zeros((1, n)) for _ in range(3))
    case, seg, steps = np.full((1, n), -1), np.full((1, n), -1), {}
    for q, i in enumerate(take):
        x[0, 2 * q], y[0, 2 * q], th[0, 2 * q] = T.a[i]
        x[0, 2 * q + 1], y[0, 2 * q + 1], th[0, 2 * q + 1] = T.b[i]
        case[0, 2 * q], seg[0, 2 * q], steps[i] = i, i, 2 * q
    return Batch(x, y, th, np.array([n], np.int32), _tables(T, list(take), n_steps=n, steps=steps), case, seg)


def member_batch(T, origin):
    """The dynamic slots of one origin for the ensemble: one trajectory per slot, the slot's poses at 2 p and 2 p + 1 behind poses that
    stand FAR away, member 0 the + version and member 1 the - version of every slot (containment: the same in both)."""
    idx = T.select(static=False, scene=origin)
    slots = sorted({int(s) for s in T.slot[idx]})
    K = len(slots)
    n = 2 * (int(T.pos[idx].max()) + 1)
    x, y, th = np.full((K, n), ORIGINS[origin][0] - FAR), np.full((K, n), ORIGINS[origin][1] - FAR), np.zeros((K, n))
    case = np.full((2, K, n), -1)
    lengths = np.zeros(K, np.int32)
    members = np.full((2, K, n, 5), np.nan)
    for k, s in enumerate(slots):
        cs = idx[T.slot[idx] == s]
        p = int(T.pos[cs[0]])
        i0 = cs[0]
        x[k, 2 * p], y[k, 2 * p], th[k, 2 * p] = T.a[i0]
        x[k, 2 * p + 1], y[k, 2 * p + 1], th[k, 2 * p + 1] = T.b[i0]
        lengths[k] = 2 * p + 2
        for m in range(2):
            i = cs[0] if len(cs) == 1 else cs[T.sign[cs] == (1 if m == 0 else -1)][0]
            members[m, k, 2 * p] = T.row[i, :5]
            case[m, k, 2 * p] = i
    b = Batch(x, y, th, lengths, ObstacleTables(), case, case, members)
    return b


def static_batches(T, scene, pad_static=0):
    """(poses batch 1 x n, swept batch K x 2) of one static scene"""
    idx = T.select(static=True, scene=scene)
    n = len(idx) + 2
    o = ORIGINS[int(T.oi[idx[0]])]
    x, y, th = np.full((1, n), o[0] - FAR), np.full((1, n), o[1] - FAR), np.zeros((1, n))
    x[0, :len(idx)], y[0, :len(idx)], th[0, :len(idx)] = T.a[idx, 0], T.a[idx, 1], T.a[idx, 2]
    case = np.full((1, n), -1)
    case[0, :len(idx)] = idx
    obs = _tables(T, list(idx), pad_static=pad_static)
    poses = Batch(x, y, th, np.array([n], np.int32), obs, case, np.full((1, n), -1))
    K = len(idx)
    case2, seg2, case_b = np.full((K, 2), -1), np.full((K, 2), -1), np.full((K, 2), -1)
    case2[:, 0], seg2[:, 0], case_b[:, 1] = idx, idx, idx
    swept = Batch(np.stack((T.a[idx, 0], T.b[idx, 0]), 1), np.stack((T.a[idx, 1], T.b[idx, 1]), 1), np.stack((T.a[idx, 2], T.b[idx, 2]), 1),
                  np.full(K, 2, np.int32), obs, case2, seg2, case_b=case_b)
    return poses, swept


def single_tables(T, i):
    """the obstacle of case i alone (dynamic: present at time index 0)"""
    if T.static[i]:
        return _tables(T, [i])
    return ObstacleTables(dyn_obb=T.row[i, :5][None, None, :], dyn_t0=0)


# ---- obstacles against the poses of a plan -----------------------------------------------------------------------------------------
def place(names, x, y, th, delta):
    """The obstacle rows (NaN-padded to 6 doubles: rectangle 5, triangle 6, circle 3) of the variants `names` whose gap to the ego
    rectangle of the rear-axle poses (x, y, th: longdoubles, or doubles) is `delta` metres, to the rounding of their coordinates."""
    vs = [next(q for q in VARIANTS if q.name == nm) for nm in names]
    assert all(v.second is None and not v.fixed for v in vs)
    t = Table()
    t.kind = np.array([v.kind for v in vs])
    t._base, t._dir = np.array([v.base for v in vs]).astype(LD), np.array([v.dir for v in vs])
    t._shape = np.array([(tuple(v.shape) + (0.0, 0.0, 0.0))[:3] if v.kind != "tri" else (0.0, 0.0, 0.0) for v in vs])
    t._tri = np.array([v.shape if v.kind == "tri" else ((0.0, 0.0),) * 3 for v in vs])
    E = ego_box(np.asarray(x, LD), np.asarray(y, LD), np.asarray(th, LD))
    frame = (E.cx.ld(), E.cy.ld(), E.ux.ld(), E.uy.ld())
    phi = np.asarray(np.arctan2(frame[3], frame[2]) + t._shape[:, 0].astype(LD), dtype=np.float64)
    os_, oc_ = dd.sincos(_d(phi))
    lo, hi = np.array([v.bracket[0] for v in vs], LD), np.array([v.bracket[1] for v in vs], LD)
    rows = np.full((len(vs), 6), np.nan)
    for kind in ("rect", "tri", "circ"):
        idx = np.flatnonzero(t.kind == kind)
        if len(idx):
            t0 = _bisect(t, idx, E.take(idx), frame, (oc_[idx], os_[idx]), lo[idx], hi[idx], np.ones(len(idx), bool))
            rows[idx] = _row_of(t, idx, _obstacle_at(t, idx, frame, t0 + np.asarray(delta, LD)[idx]), phi)
    return rows


def gaps_to_row(row, x, y=None, th=None):
    """gaps [m] (longdouble) of the ego rectangles of the rear-axle poses x, y, th [m] (or of the Box x) to ONE obstacle row (5, 6 or 3
    doubles)"""
    E = x if isinstance(x, Box) else ego_box(np.asarray(x, LD), np.asarray(y, LD), np.asarray(th, LD))
    row = np.asarray(row, float)[None, :]
    if row.shape[1] == 5:
        return gap_rect(E, rect_box(row)).ld()
    if row.shape[1] == 6:
        return gap_tri(E, [_d(row[:, 2 * k]) for k in range(3)], [_d(row[:, 2 * k + 1]) for k in range(3)]).ld()
    return gap_circ(E, _d(row[:, 0]), _d(row[:, 1]), _d(row[:, 2])).ld()


# Planner labels: three of tests/_xref.py's cases -- straight, curved, and one whose candidates run the horizon extension (time sample
# 4.3 s of a 6.3 s horizon) -- each on the block of candidates of one time sample; the ego poses are the extended-precision
# reference's rows (x, y, theta), never the device's.
PLANNER_CASES = {"straight_keep_n16": 3, "arc_keep_n17": 3, "scurve_stop_n64": 2}     # name -> index of the time sample
PLANNER_GAPS = (1e-8, -1e-8, 1e-6, -1e-6)
PLANNER_FORMS = {   # form -> the variants it rotates through
    # (dynamic: the overlapping ones are those whose bounding circle is tight -- corner to corner; a strip of NO width end-on)
    "dynamic": ("d_square", "c_front_left", "a_left_upright", "f_end_on_diagonal_hw0"),
    "folded": ("f_end_on_diagonal", "c_front_right_thin", "b_its_corner", "f_far_end_normal_on_diagonal"),
    "unfolded": ("f_end_on_diagonal", "c_front_right_thin", "b_its_corner", "f_far_end_normal_on_diagonal"),
    "grid_of_five": ("f_far_end_normal_on_diagonal", "f_end_on_diagonal_hw0", "c_rear_left_square", "d_rear_oblong"),
    "triangle": ("g_edge_through_corner", "g_100m_edge", "g_collinear_end", "g_vertex_on_edge_clockwise"),
    "circle": ("h_on_corner", "h_point_on_edge", "h_on_edge", "h_point_on_corner"),
}
LEFT_OUT_BELOW = 1e-9        # metres: a candidate whose smallest gap is closer to contact than this is not compared
# (the rows' allowance -- _xref.ORACLE_BOUND, 1e-11 m -- plus B at these coordinates, 2e-12 m, is 800 times below the smallest gap)


@dataclasses.dataclass
class Scene:
    form: str
    variant: str
    gap: float
    target: tuple            # (candidate index within the block, step)
    tables: ObstacleTables
    fold_static: int         # the option's value for this scene
    label: np.ndarray        # [m] 3 colliding | 1 free | 0 not asked (no feasible candidate)
    decided: np.ndarray      # [m] bool
    gmin: np.ndarray         # [m] the smallest gap over the candidate's steps and the shapes


@functools.lru_cache(maxsize=None)
def planner_scenes(name):
    """(lo, hi, scenes) of one case: the candidates lo .. hi - 1 and, per form and gap, one obstacle placed against a chosen
    (candidate, step) pose -- the extreme feasible lateral samples are among the chosen."""
    import _xref as X
    c = X.case(name)
    nL, nD = len(c.inp.L), len(c.inp.D)
    lo = PLANNER_CASES[name] * nL * nD
    hi = lo + nL * nD
    feasible = (X.oracle_run(name)[0][lo:hi] & 3) == 1
    ref = X.reference_for(name, tuple(range(lo, hi)))
    n = c.inp.params.N + 1
    px, py, pth = (ref.states[:, r, :] for r in (X.X, X.Y, X.THETA))           # [m, n] longdouble
    assert c.inp.params.factor == 1 and np.isfinite(np.asarray(px[feasible], float)).all()
    iD = np.arange(hi - lo) % nD
    cand = np.flatnonzero(feasible)
    left, right = cand[iD[cand] == iD[cand].min()], cand[iD[cand] == iD[cand].max()]
    chosen = [int(left[0]), int(right[-1]), int(cand[len(cand) // 2]), int(left[-1]), int(right[0])]
    steps = [n - 1, n // 2, 1, n - 2, (2 * n) // 3]
    t0 = int(c.inp.params.time_step0)
    far = np.array([c.co.reference[0, 0] - FAR, c.co.reference[0, 1] - FAR, 0.3, 2.0, 1.0])
    scenes = []
    boxes = ego_box(px.ravel(), py.ravel(), pth.ravel())
    plan = [(form, variants[gi], gap, chosen[(fi + gi) % len(chosen)], steps[(fi + 2 * gi) % len(steps)])
            for fi, (form, variants) in enumerate(PLANNER_FORMS.items()) for gi, gap in enumerate(PLANNER_GAPS)]
    ks, is_ = np.array([q[3] for q in plan]), np.array([q[4] for q in plan])
    placed = place([q[1] for q in plan], px[ks, is_], py[ks, is_], pth[ks, is_], [q[2] for q in plan])
    for (form, vname, gap, k, i), row in zip(plan, placed):
        row = row[~np.isnan(row)]
        dyn = np.full((1, n, 5), np.nan)
        dyn[0, :] = far                                    # a dynamic table that is there, with an obstacle that is not near
        if form in ("folded", "unfolded"):
            dyn[0, :, 3] = 45.0                            # ... and larger than the rectangle: a larger rectangle is not folded
        g = gaps_to_row(row, boxes).reshape(hi - lo, n)
        kw = {}
        if form == "dynamic":
            dyn = np.concatenate((dyn, np.full((1, n, 5), np.nan)))
            dyn[1, i] = row                                # present at that step only
            g = g[:, i:i + 1]
        elif form in ("folded", "unfolded"):
            kw["static_obb"] = [row]
        elif form == "grid_of_five":
            kw["static_obb"] = [far + [10.0 * q, 0, 0, 0, 0] for q in range(1, 3)] + [row] + [far + [10.0 * q, 0, 0, 0, 0] for q in range(3, 5)]
        elif form == "triangle":
            kw["static_tri"] = [row]
        else:
            kw["static_circ"] = [row]
        gmin = np.asarray(g.min(axis=1), float)
        decided = feasible & (np.abs(gmin) >= LEFT_OUT_BELOW)
        label = np.where(feasible, np.where(gmin <= 0, 3, 1), 0)
        scenes.append(Scene(form, vname, gap, (k, i), ObstacleTables(dyn_obb=dyn, dyn_t0=t0, **kw), 0 if form == "unfolded" else -1,
                            label, decided, gmin))
    return lo, hi, tuple(scenes)


# ---- exactly touching ------------------------------------------------------------------------------------------------------------
# Closed sets: g = 0 is a hit.  The table cannot hold such a case (|g| >= 8 B); these few are exact in doubles AND in the formulas --
# heading 0 on both sides, dyadic numbers, the reference point in the rectangle's centre -- so that `>` and `>=` differ on them.
EXACT_HL, EXACT_HW = 2.0, 0.75
EXACT_ORIGINS = ((0.0, 0.0), (1024.0, -512.0), (float(2 ** 21), -float(2 ** 20)))
EXACT_ROWS = ((5.0, 0.0, 0.0, 1.0, 0.5), (0.0, 1.25, 0.0, 1.0, 0.5), (3.0, 1.25, 0.0, 1.0, 0.5), (-3.5, -1.0, 0.0, 1.5, 0.25))   # ego at (2, 0) | (0, 0) ...
EXACT_EGO = ((2.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0))


def exact_params(n=2):
    return make_params(dt=0.1, N=n - 1, factor=1, time_step0=0, low_vel_mode=False, lon_mode=0, constraint_mask=0, flags=0, x0_lon=[0, 0, 0],
                       x0_lat=[0, 0, 0], x0_orientation=0.0, wheelbase=2.5, wb_rear_axle=0.0, length=2 * EXACT_HL, width=2 * EXACT_HW,
                       a_max=11.5, v_switch=7.319, delta_max=1.066, v_delta_max=0.4)


def exact_cases():
    """(ego x, y [m]; rows [m, 5]): touching rectangles, 400 m apart, whose gap is exactly 0 in this reference"""
    ex, ey, rows = [], [], []
    for oi, (ox, oy) in enumerate(EXACT_ORIGINS):
        for q, (row, ego) in enumerate(zip(EXACT_ROWS, EXACT_EGO)):
            sx = ox + 512.0 * q
            ex.append(sx + ego[0])
            ey.append(oy + ego[1])
            rows.append((sx + row[0], oy + row[1]) + row[2:])
    ex, ey, rows = np.array(ex), np.array(ey), np.array(rows)
    g = gap_rect(ego_box(ex, ey, np.zeros(len(ex)), EXACT_HL, EXACT_HW, 0.0), rect_box(rows))
    assert np.all(g.hi == 0) and np.all(g.lo == 0), "not exactly touching"
    return ex, ey, rows


# ---- the double predicate's own error --------------------------------------------------------------------------------------------
def oracle_verdicts(T):
    """(pose verdict, swept verdict) of oracle.check_poses / oracle.check_swept on every case, its obstacle alone"""
    from oracle import oracle
    s = np.arange(0.0, 8.0, 1.0)
    pose, swept = np.zeros(len(T), bool), np.zeros(len(T), bool)
    p = params()
    for i in range(len(T)):
        tb = oracle.OracleTables(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0, single_tables(T, i))
        xs, ys, ths = [T.a[i, 0], T.b[i, 0]], [T.a[i, 1], T.b[i, 1]], [T.a[i, 2], T.b[i, 2]]
        pose[i] = oracle.check_poses(p, tb, xs[:1], ys[:1], ths[:1])[0][0]
        swept[i] = oracle.check_swept(p, tb, xs, ys, ths)[0] == 0
    return pose, swept


def oracle_worst_error(L=None):
    """{(family, origin): (cases, wrong verdicts, largest |g| of a wrong verdict in u scale)} of the double oracle on the ladder"""
    L = L if L is not None else ladder_table()
    pose, swept = oracle_verdicts(L)
    wrong = (swept != L.hit) | (~L.swept & (pose != L.hit_pose))
    units = np.abs(np.asarray(L.g, float)) / (L.B / BAND)
    out = {}
    for f in FAMILIES:
        for oi in range(len(ORIGINS)):
            m = (L.family == f) & (L.oi == oi)
            if m.any():
                out[(f, oi)] = (int(m.sum()), int((wrong & m).sum()), float(units[wrong & m].max()) if (wrong & m).any() else 0.0)
    return out


def device_results(T):
    """{path: [N] bool, a wrong verdict of the device on the case} on GPU 0 -- librp_check (the pose flag of every case in the ragged
    batches; first pose and first segment of every case: dynamic cases as one trajectory each, static ones as two poses),
    librp_ensemble (first pose and first segment per member), librp_clearance (0 <=> hit, within B elsewhere) and rp_check_swept
    (every case, one call each)."""
    from commonroad_rp_amd._capi import RpContext
    from commonroad_rp_amd.clearance import ClearanceQuery
    from commonroad_rp_amd.ensemble_check import EnsembleChecker
    from commonroad_rp_amd.trajectory_check import TrajectoryChecker
    N = len(T)
    wrong = {k: np.zeros(N, bool) for k in ("check", "ensemble", "clearance", "check_swept")}

    def mark(path, cases, bad):
        np.logical_or.at(wrong[path], cases[cases >= 0], bad[cases >= 0])
    with TrajectoryChecker(0) as ck, EnsembleChecker(0) as en, ClearanceQuery(0) as cl:
        for o in range(len(ORIGINS)):
            b = dynamic_batch(T, o)
            p = params(n=b.x.shape[1])
            ck.set_obstacles(b.obstacles)
            r = ck.check(p, b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=True, want_pose_hits=True)
            mark("check", b.case, r.pose_hits != b.expected(T)[0])
            cb = case_batch(T, o)
            r = ck.check(params(n=cb.x.shape[1]), cb.x, cb.y, cb.th, lengths=cb.lengths, poses=True, swept=True)
            mark("check", cb.case.max(axis=1), (r.first_pose_hit != cb.expected(T)[1]) | (r.first_segment_hit != cb.expected(T)[2]))
            cl.set_obstacles(b.obstacles)
            c = cl.query(p, b.x, b.y, b.th, lengths=b.lengths, want_pose_clearance=True).pose_clearance
            i = np.maximum(b.case, 0)
            mark("clearance", b.case, ((c == 0.0) != T.hit_pose[i]) | (~T.hit_pose[i] & ~(np.abs(c - np.asarray(T.dist[i], float)) <= T.B_pose[i])))
            m = member_batch(T, o)
            en.set_obstacles(ObstacleTables(), members=m.members, dyn_t0=0)
            r = en.check(params(n=m.x.shape[1]), m.x, m.y, m.th, lengths=m.lengths, poses=True, swept=True)
            at = m.case.max(axis=2)
            for q in range(2):
                mark("ensemble", at[q], ((r.first_pose_hit[:, q] >= 0) != T.hit_pose[at[q]]) | ((r.first_segment_hit[:, q] >= 0) != T.hit[at[q]]))
        for sc in range(T.n_static_scenes):
            poses, swept = static_batches(T, sc)
            for b in (poses, swept):
                p, two = params(n=b.x.shape[1]), b.x.shape[1] == 2
                ck.set_obstacles(b.obstacles)
                r = ck.check(p, b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=two, want_pose_hits=True)
                mark("check", b.case, r.pose_hits != b.expected(T)[0])
                en.set_obstacles(b.obstacles)
                e = en.check(p, b.x, b.y, b.th, lengths=b.lengths, poses=True, swept=two)
                if two:
                    mark("check", b.seg_case[:, 0], r.first_segment_hit != b.expected(T)[2])
                    mark("ensemble", b.seg_case[:, 0], (e.first_pose_hit[:, 0] != b.expected(T)[1]) | (e.first_segment_hit[:, 0] != b.expected(T)[2]))
                else:
                    cl.set_obstacles(b.obstacles)
                    c = cl.query(p, b.x, b.y, b.th, want_pose_clearance=True).pose_clearance
                    i = np.maximum(b.case, 0)
                    mark("clearance", b.case, ((c == 0.0) != T.hit_pose[i]) | (~T.hit_pose[i] & ~(np.abs(c - np.asarray(T.dist[i], float)) <= T.B_pose[i])))
    ctx = RpContext(0)
    s = np.arange(0.0, 8.0, 1.0)
    ctx.set_reference(s, 0 * s, 0 * s, 0 * s, np.stack((s, 0 * s), 1), 20.0)
    p = params(n=2)
    for i in range(N):
        ctx.set_obstacles(single_tables(T, i))
        wrong["check_swept"][i] = (ctx.check_swept(p, [T.a[i, 0], T.b[i, 0]], [T.a[i, 1], T.b[i, 1]], [T.a[i, 2], T.b[i, 2]]) == 0) != T.hit[i]
    ctx.close()
    return wrong


PLANNER_PATHS = ("single_launch", "two_kernel", "g32", "g64")


def planner_run(ctx, name, draw):
    """rp_plan on every scene of a case, on the context as its options stand (eager collision path; "fold_static" as the scene says)
    -> per scene (scene, labels [m], n_collision, (collision level, a folded table exists, lanes, single launch), launch)"""
    import _xref as X
    from commonroad_rp_amd._capi import COLLISION_EAGER, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL, FLAG_SKIP_COLLISION
    lo, hi, scenes = planner_scenes(name)
    c = X.case(name)
    inp = X.with_flags(c.inp, set_=(FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL) if draw else 0, clear=FLAG_SKIP_COLLISION | FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)
    ctx.set_collision_path(COLLISION_EAGER)
    ctx.set_coordinate_system(c.co)
    out = []
    try:
        for s in scenes:
            ctx.set_obstacles(s.tables)
            ctx.set_option("fold_static", s.fold_static)
            res = ctx.plan(inp, lo, hi)
            lab = ctx.fetch_status()[0] & 3
            launch = X.launch_of(ctx)
            out.append((s, lab, int(res.n_collision), (ctx.get_option("last_collision_level"), ctx.get_option("fold_static_steps") > 0) + launch[1:3], launch))
    finally:
        ctx.set_option("fold_static", -1)
    return out


def planner_results():
    """{launch path: (decided labels compared, wrong ones)} of rp_plan over the scenes of PLANNER_CASES, production and draw mode, on GPU 0"""
    from _paths import launch_path_env
    from commonroad_rp_amd._capi import RpContext
    res = {}
    for path in PLANNER_PATHS:
        n = bad = 0
        with launch_path_env(path):
            ctx = RpContext(0)
            try:
                for name in PLANNER_CASES:
                    for draw in (False, True):
                        for s, lab, _, _, _ in planner_run(ctx, name, draw):
                            n += int(s.decided.sum())
                            bad += int((s.decided & (lab != s.label)).sum())
            finally:
                ctx.close()
        res[path] = (n, bad)
    return res


def summary_lines(T, worst, device=None):
    lines = ["family origin  cases  min|g|/B  oracle: ladder cases  wrong  worst wrong |g| [u scale]" +
             ("  wrong device verdicts: " + " / ".join(device) if device else "")]
    gB = np.abs(np.asarray(T.g, float)) / T.B
    for f in FAMILIES:
        for oi in range(len(ORIGINS)):
            m = (T.family == f) & (T.oi == oi)
            n, w, e = worst.get((f, oi), (0, 0, 0.0))
            lines.append(f"{f:>6} {oi:>6} {int(m.sum()):>6} {gB[m].min():>9.3g} {n:>21} {w:>6} {e:>10.3f}" + ("  " + " / ".join(str(int((w & m).sum())) for w in device.values()) if device else ""))
    return lines


def main(argv):
    if not HAVE_LONGDOUBLE:
        raise SystemExit(SKIP_REASON)
    T = table()
    worst = oracle_worst_error()
    pose, swept = oracle_verdicts(T)
    device = plans = gpu = None
    try:
        import torch
        if torch.cuda.device_count() > 0:
            gpu = torch.cuda.get_device_name(0)
            device, plans = device_results(T), planner_results()
    except ImportError:
        pass
    text = [f"{len(T)} cases, B = {BAND:g} u scale, u = 2^-53; every case |g| >= {DECIDED:g} B; reference and double oracle: CPU; " +
            (f"device columns: measured on {gpu}" if device else "no GPU here: no device columns"),
            f"oracle verdicts on the table: {int((swept != T.hit).sum() + (pose != T.hit_pose).sum())} wrong",
            f"ladder: contacts displaced by +- k u scale, k in {LADDER}"] + summary_lines(T, worst, device)
    big = max(e for _, _, e in worst.values())
    text.append(f"worst wrong |g| over all families: {big:.3f} u scale; B / 4 = {BAND / 4:g} u scale: " +
                ("no family exceeds it, B stays 8 u scale" if big <= BAND / 4 else "EXCEEDED: that family's band becomes 4 x its worst"))
    if plans:
        text.append("rp_plan, obstacles +-1e-8 and +-1e-6 m from chosen poses of the extended-precision rows (" + ", ".join(PLANNER_CASES) +
                    f"; {len(PLANNER_FORMS)} obstacle forms; production and draw mode): wrong labels / decided labels compared, per launch path")
        text += [f"{path:>14}  {bad} / {n}" for path, (n, bad) in plans.items()]
    out = "\n".join(text) + "\n"
    if len(argv) > 1:
        with open(argv[1], "w") as fh:
            fh.write(out)
    print(out, end="")


if __name__ == "__main__":
    main(sys.argv)
