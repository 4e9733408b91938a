"""What only the plumbing the seven trajectory libraries share can get wrong (csrc/rp_session.h, commonroad_rp_amd/_session.py): the
blocks of a call that grow, a table that replaces an earlier one, a refused set call, and two objects side by side.  The yardstick is
the library itself: whatever an object returns after such a history is bit-equal to what a FRESH object of the class returns for that
call with those tables.  That the libraries compute the right thing is the business of their own tests.

Cases: the inputs the siblings' helpers build (tests/_clearance.py, _ensemble.py, _score.py, _lift.py, _pick.py, _epick.py).
  small  2 x 3       the first two trajectories and three poses of the big call
  big                input and result blocks beyond the 65536-byte floor of a block: 1100 x 64 poses for the checkers and the clearance
                     query (the checker's result block grows with the per-pose flags only), 257 x 65 for the scorer, 37 x 65 for the
                     lifter and the picks (six input planes, eight planes back)
Tables A and B differ in every kind a class holds; that their results differ is asserted, or a test could not tell them apart.
"""
import dataclasses
import functools

import numpy as np
import pytest

from commonroad_rp_amd import _capi
from commonroad_rp_amd.collision import ObstacleTables

import _clearance as CL
import _ensemble as E
import _epick as EP
import _lift as L
import _pick as P
import _score as S

pytestmark = pytest.mark.gpu
EINVAL = -1


# ---- the seven classes: what they hold, how a call is made, which set calls are refused ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _poses():
    """1100 x 64 poses with ragged lengths, obstacle tables A around them and B, one circle on the first pose of trajectory 0"""
    x, y, th, lengths, t0, obs = CL.random_batch(np.random.default_rng(65), 1100, 64, 5, 6, True, 3.0, 3.0)
    other = ObstacleTables(static_circ=[[x[0, 0], y[0, 0], 1.0]], dyn_obb=obs.dyn_obb[:2, 5:] + 0.25, dyn_t0=obs.dyn_t0 + 2)
    rng = np.random.default_rng(66)
    members = {"A": E.make_members(rng, obs.dyn_obb)(8), "B": E.make_members(rng, other.dyn_obb)(2)}   # (1100 x 8 verdicts: two matrices of 35200 B)
    return dict(x=x, y=y, th=th, lengths=lengths, p=CL._params(time_step0=t0, factor=1, n=64), obs={"A": obs, "B": other}, members=members)


def _cut(size, planes, lengths):
    """The planes and lengths of a call: all of them, or trajectories 0, 1 and poses 0 .. 2"""
    if size == "big":
        return planes, lengths
    return [None if q is None else np.ascontiguousarray(q[:2, :3]) for q in planes], None if lengths is None else np.minimum(lengths[:2], 3)


class Checker:
    kinds = ("obstacles",)

    def make(self):
        from commonroad_rp_amd import TrajectoryChecker
        return TrajectoryChecker(0)

    def set(self, o, kind, v):
        o.set_obstacles(_poses()["obs"][v])

    def call(self, o, size):
        c = _poses()
        (x, y, th), lens = _cut(size, (c["x"], c["y"], c["th"]), c["lengths"])
        return o.check(c["p"], x, y, th, lengths=lens, poses=True, swept=True, want_pose_hits=True)

    def refused(self, o):
        return [o._lib.rp_checker_set_obstacles(o._h, -1, None, 0, None, 0, None, 0, 0, 0, None)]


class Clearance(Checker):
    def make(self):
        from commonroad_rp_amd import ClearanceQuery
        return ClearanceQuery(0)

    def call(self, o, size):
        c = _poses()
        (x, y, th), lens = _cut(size, (c["x"], c["y"], c["th"]), c["lengths"])
        return o.query(c["p"], x, y, th, lengths=lens, cutoff=CL.CUTOFF, margin=CL.MARGIN, want_pose_clearance=True)

    def refused(self, o):
        return [o._lib.rp_clearance_set_obstacles(o._h, 0, None, -1, None, 0, None, 0, 0, 0, None)]


class Ensemble:
    kinds = ("static", "members")

    def make(self):
        from commonroad_rp_amd import EnsembleChecker
        return EnsembleChecker(0)

    def set(self, o, kind, v):
        c = _poses()
        if kind == "static":
            o.set_static(c["obs"][v])
        else:
            o.set_members(c["members"][v], c["obs"][v].dyn_t0)

    def call(self, o, size):
        c = _poses()
        (x, y, th), lens = _cut(size, (c["x"], c["y"], c["th"]), c["lengths"])
        return o.check(c["p"], x, y, th, lengths=lens, poses=True, swept=True, max_members_hit=1)

    def refused(self, o):
        return [o._lib.rp_ensemble_set_static(o._h, 0, None, 0, None, -1, None), o._lib.rp_ensemble_set_members(o._h, 0, 0, 0, 0, None),
                o._lib.rp_ensemble_set_members(o._h, 2, -1, 4, 0, None)]


class Scorer:
    kinds = ("reference",)

    def make(self):
        from commonroad_rp_amd import TrajectoryScorer
        return TrajectoryScorer(0)

    def set(self, o, kind, v):
        c = S.shape_case("n65_k257")
        o.set_reference(*((c.ref, c.ref_pos, c.ref_theta) if v == "A" else S.path("cfg2")), c.d_limit)

    def call(self, o, size):
        c = S.shape_case("n65_k257")
        (x, y, th, v, a, kappa), lens = _cut(size, (c.x, c.y, c.theta, c.v, c.a, c.kappa), c.lengths)
        return o.score(c.p, c.cost, x, y, th, v=v, a=a, kappa=kappa, lengths=lens, want_states=True)

    def refused(self, o):
        return [o._lib.rp_score_set_reference(o._h, 1, None, None, None, 20.0)]


def _paths():
    return {"A": L.case("ragged").path, "B": L.case("long_path").path}


class Lifter(Scorer):
    def make(self):
        from commonroad_rp_amd import TrajectoryLifter
        return TrajectoryLifter(0)

    def set(self, o, kind, v):
        o.set_reference(*L.table_args(_paths()[v]))

    def call(self, o, size):
        c = L.case("ragged")
        planes, lens = _cut(size, c.planes, c.lengths)
        return o.lift(c.p, *planes, lengths=lens, theta0=c.theta0)

    def refused(self, o):
        return [o._lib.rp_lift_set_reference(o._h, 1, None, None, None, None, None, 20.0)]


class Picker:
    kinds = ("reference", "obstacles")

    def make(self):
        from commonroad_rp_amd import TrajectoryPicker
        return TrajectoryPicker(0)

    def set(self, o, kind, v):
        if kind == "reference":
            o.set_reference(*L.table_args(_paths()[v]))
        else:
            o.set_obstacles(P.case("ragged").obs if v == "A" else P.case("many_static").obs)

    def call(self, o, size):
        c = P.case("ragged")
        planes, lens = _cut(size, c.planes, c.lengths)
        return o.pick(c.p, c.cost, *planes, lengths=lens, theta0=c.theta0, poses=True, swept=True, want_planes=True, want_hits=True)

    def refused(self, o):
        return [o._lib.rp_pick_set_reference(o._h, 1, None, None, None, None, None, 20.0),
                o._lib.rp_pick_set_obstacles(o._h, 0, None, 0, None, 0, None, -1, 3, 0, None)]


class EnsemblePicker:
    kinds = ("reference", "static", "members")

    def make(self):
        from commonroad_rp_amd import EnsemblePicker
        return EnsemblePicker(0)

    def set(self, o, kind, v):
        c = EP.multi("ragged_m9")
        if kind == "reference":
            o.set_reference(*L.table_args(_paths()[v]))
        elif kind == "static":
            o.set_static(c.obs if v == "A" else P.case("many_static").obs)
        elif v == "A":
            o.set_members(c.members, c.dyn_t0, weights=np.linspace(0.05, 0.2, c.M))
        else:
            o.set_members(c.members[1:3], c.dyn_t0 + 1)

    def call(self, o, size):
        c = EP.multi("ragged_m9")
        planes, lens = _cut(size, c.planes, c.lengths)
        return o.pick(c.p, c.cost, *planes, lengths=lens, theta0=c.theta0, poses=True, swept=True, max_risk=0.3, want_planes=True, want_hits=True)

    def refused(self, o):
        return [o._lib.rp_epick_set_reference(o._h, 1, None, None, None, None, None, 20.0), o._lib.rp_epick_set_static(o._h, -1, None, 0, None, 0, None),
                o._lib.rp_epick_set_members(o._h, 0, 0, 0, 0, None, None), o._lib.rp_epick_set_members(o._h, 1, 2, 3, 0, None, None)]


CLASSES = {"checker": Checker(), "ensemble": Ensemble(), "clearance": Clearance(), "scorer": Scorer(), "lifter": Lifter(), "picker": Picker(),
           "ensemble_picker": EnsemblePicker()}


# ---- the yardstick: a fresh object, those tables, that call alone -----------------------------------------------------------------------
def _load(a, o, tables):
    for kind, v in zip(a.kinds, tables):
        a.set(o, kind, v)


@functools.lru_cache(maxsize=None)
def _fresh(name, tables, size):
    a = CLASSES[name]
    with a.make() as o:
        _load(a, o, tables)
        return a.call(o, size)


def _same(got, want):
    """Every array and scalar of two results equal bit for bit (NaN included); the first field that is not, or None"""
    for f in dataclasses.fields(want):
        x, y = getattr(got, f.name), getattr(want, f.name)
        if x is None or y is None:
            if x is not y:
                return f.name
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return f.name
    return None


def _all(a, v):
    return tuple(v for _ in a.kinds)


def _variants(a):
    """Table sets that differ from all-A in one kind each, and all-B"""
    one = [tuple("B" if k == kind else "A" for k in a.kinds) for kind in a.kinds]
    return list(dict.fromkeys(one + [_all(a, "B")]))


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLASSES))
def test_blocks_regrow_and_shrunk_calls_read_their_own_part(name):
    """small, big, small on one object: each equals the call alone on a fresh object"""
    a = CLASSES[name]
    A = _all(a, "A")
    with a.make() as o:
        _load(a, o, A)
        for size in ("small", "big", "small"):
            assert _same(a.call(o, size), _fresh(name, A, size)) is None, size
    assert _same(_fresh(name, A, "small"), _fresh(name, A, "big")) is not None


@pytest.mark.parametrize("name", list(CLASSES))
def test_a_table_replaces_the_earlier_one(name):
    """A, B, A in every kind of table a class holds: the results are a fresh object's with those tables, and B's are not A's"""
    a = CLASSES[name]
    A = _all(a, "A")
    with a.make() as o:
        _load(a, o, A)
        assert _same(a.call(o, "big"), _fresh(name, A, "big")) is None
        for tables in _variants(a):
            assert _same(_fresh(name, tables, "big"), _fresh(name, A, "big")) is not None, tables
            _load(a, o, tables)
            assert _same(a.call(o, "big"), _fresh(name, tables, "big")) is None, tables
            _load(a, o, A)
            assert _same(a.call(o, "big"), _fresh(name, A, "big")) is None, tables


@pytest.mark.parametrize("name", list(CLASSES))
def test_a_refused_set_call_leaves_the_tables_in_force(name):
    a = CLASSES[name]
    B = _all(a, "B")
    with a.make() as o:
        _load(a, o, B)
        codes = a.refused(o)
        assert len(codes) >= len(a.kinds) and codes == [EINVAL] * len(codes)
        assert _same(a.call(o, "big"), _fresh(name, B, "big")) is None
        # ... and through the binding the refusal is an RpError that carries the code and the library's message
        with pytest.raises(_capi.RpError, match=r"set_\w+ -> -1: rp_\w+: "):
            if "reference" in a.kinds:
                o.set_reference(np.zeros((1, 2)), *([np.zeros(1)] * (2 if name == "scorer" else 4)))
            elif "members" in a.kinds:
                o.set_members(np.zeros((0, 1, 1, 5)))
            else:
                o._call("set_obstacles", -1, None, 0, None, 0, None, 0, 0, 0, None)   # (no ObstacleTables has a negative count)
        assert _same(a.call(o, "small"), _fresh(name, B, "small")) is None


@pytest.mark.parametrize("name", list(CLASSES))
def test_two_objects_keep_their_own_tables(name):
    """Two objects of one class alive at once, tables A and B, calls interleaved: neither sees the other's tables or blocks"""
    a = CLASSES[name]
    A, B = _all(a, "A"), _all(a, "B")
    with a.make() as first, a.make() as second:
        for kind in a.kinds:   # (set calls interleaved too)
            a.set(first, kind, "A")
            a.set(second, kind, "B")
        for size in ("big", "small", "big"):
            got_first, got_second = a.call(first, size), a.call(second, size)
            assert _same(got_first, _fresh(name, A, size)) is None, size
            assert _same(got_second, _fresh(name, B, size)) is None, size
        _load(a, second, A)   # replacing the second one's tables leaves the first one's results where they were
        assert _same(a.call(first, "big"), _fresh(name, A, "big")) is None
        assert _same(a.call(second, "big"), _fresh(name, A, "big")) is None
