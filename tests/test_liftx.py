"""librp_lift, librp_pick and librp_epick against the extended-precision reference of tests/_liftx.py: the eight lifted planes and the
picks' costs.  Needs a real MI355X: ``pytest -m gpu``.

No tolerance here is taken from the device: a plane may be MARGIN_MAX = 8 times as far from the reference as the double oracle
(``_lift.reference``) is, plus 8 spacings of the plane's scale, and 4 times in the root mean square plus 2 spacings; a cost 8 times the
oracle's relative distance plus the summation bound of the trajectory's length (the rule: tests/_xref.py, its use here:
tests/_liftx.py).  Compared are the poses on which the oracle holds a number; NaN patterns, status words and reductions stay with
tests/test_lift.py, test_pick.py and test_epick.py.  What the oracle's own distance is, which trajectories are left out, that the new
families meet their conditions and that the comparison fails on planted defects: tests/test_liftx_abi.py, without a GPU.  Every test
prints E_O, E_D and their ratio per plane; ``python tests/_liftx.py`` writes them to profiles/accuracy_lift.txt."""
import numpy as np
import pytest

import _liftx as LX
import _pick as P
import _xref as X

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not X.HAVE_LONGDOUBLE, reason=X.SKIP_REASON)]
KNOWN = LX.KNOWN_EXCEEDANCES   # (case, plane) of rp_lift_evaluate on the case's own tables -> diagnosis: asserted on their own, expected to fail


@pytest.fixture(scope="module")
def lifter():
    from commonroad_rp_amd import TrajectoryLifter
    with TrajectoryLifter(0) as lf:
        yield lf


@pytest.fixture(scope="module")
def picker():
    from commonroad_rp_amd import TrajectoryPicker
    with TrajectoryPicker(0) as pk:
        yield pk


@pytest.fixture(scope="module")
def epicker():
    from commonroad_rp_amd import EnsemblePicker
    with EnsemblePicker(0) as ep:
        yield ep


_lifted = {}


def _lift_planes(lifter, name):
    """[K, 8, n] of rp_lift_evaluate on a case, run once per module"""
    if name not in _lifted:
        _lifted[name] = LX.stacked(LX.run_lift(lifter, LX.case(name)))
        _lifted[name].setflags(write=False)
    return _lifted[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _held(name, what, got, known=()):
    """the rule on one device result [K, 8, n]: every plane but those of ``known``"""
    rows, n_out, _ = LX.compare_planes(LX.reference(name).rows, LX.oracle_view(name)[0], got)
    print(f"{name}: {what} ({n_out} trajectories left out)")
    for r in rows:
        print("  " + r.line())
    found = [r.line() for r in rows if not r.ok and r.row not in known]
    assert not found, "\n".join([f"{name}, {what}:"] + found)
    return rows


@pytest.mark.parametrize("name", LX.CASE_NAMES)
def test_lift_planes(lifter, name):
    got = _lift_planes(lifter, name)
    assert got.shape == LX.oracle_view(name)[0].shape
    _held(name, "rp_lift_evaluate", got, known=[plane for case, plane in KNOWN if case == name])


@pytest.mark.parametrize("name", LX.CASE_NAMES)
def test_lift_states_and_both_table_variants(lifter, name):
    """the blocks of lift_states: the lift's planes bit for bit and the inputs; where the case's path fits both, the same call on the path
    filled up by a straight tail to LF_LDS_ROWS segments (the table staged in LDS) and to LF_LDS_ROWS + 1 (read from device memory)"""
    c = LX.case(name)
    lifter.set_reference(*LX.L.table_args(c.path))
    states = lifter.lift_states(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)
    np.testing.assert_array_equal(_bits(states[:, P.PLANE_ROWS]), _bits(_lift_planes(lifter, name)))
    for row, q in zip(P.INPUT_ROWS, c.planes):
        np.testing.assert_array_equal(_bits(states[:, row]), _bits(q))
    assert (name in LX.BOTH_VARIANTS) == LX.fits_both(name)
    if name in LX.BOTH_VARIANTS:
        for n_seg in (LX.LDS_ROWS, LX.LDS_ROWS + 1):
            lifter.set_reference(*LX.L.table_args(LX.padded(c.path, n_seg)))
            states = lifter.lift_states(c.p, *c.planes, lengths=c.lengths, theta0=c.theta0)
            _held(name, f"lift_states on {n_seg} segments", states[:, P.PLANE_ROWS])


def _held_cost(name, q, lib, got):
    c = LX.case(name)
    sel = LX.cost_selection(name)
    e_o, e_d, bound, ok = LX.compare_costs(LX.reference(name).cost[q], LX.oracle_view(name)[1 + q], got.cost, sel, c.out.lengths)
    print(f"{name}: {lib} cost {q} (kind {int(c.costs[q].kind)}): oracle {e_o:.3e} device {e_d:.3e} bound {bound:.3e} relative, {int(sel.sum())} trajectories")
    assert sel.any() and ok, (name, lib, q, e_o, e_d, bound)
    assert got.best >= 0 and _bits(np.float64(got.best_cost)) == _bits(got.cost[got.best])
    feasible = np.flatnonzero(np.isfinite(got.cost))
    assert got.best == feasible[np.argmin(got.cost[feasible])]       # (argmin: the first of equal costs)


@pytest.mark.parametrize("name", LX.COST_CASES)
def test_pick_and_epick_planes_and_costs(lifter, picker, epicker, name):
    """rp_pick_select with mode = 0 and rp_epick_select with mode = 0 and one empty member, with a default and a fail-safe rp_cost: the
    planes have the bits of the lift's of this process, the costs follow the rule, best_cost has the bits of cost[best]"""
    c = LX.case(name)
    lift = _lift_planes(lifter, name)
    for q, cost in enumerate(c.costs):
        for lib, got in (("rp_pick_select", LX.run_pick(picker, c, cost)), ("rp_epick_select", LX.run_epick(epicker, c, cost))):
            np.testing.assert_array_equal(_bits(LX.stacked(got)), _bits(lift), err_msg=f"{name}: planes of {lib}")
            assert got.n_collision == 0
            _held_cost(name, q, lib, got)


def test_cases_reach_what_they_claim():
    """worked out on the CPU from the inputs: a standstill's carry that starts on lane 63 and one that starts on lane 0, a wrap between
    two poses of one chunk and across a chunk boundary, both table variants"""
    got = vars(LX.coverage())
    assert all(got.values()), got


if KNOWN:
    @pytest.mark.parametrize("name,plane", [pytest.param(*k, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason=KNOWN[k]), id="-".join(k))
                                            for k in KNOWN])
    def test_known_exceedance(lifter, name, plane):
        """ONE plane of rp_lift_evaluate on a case's own tables that exceeds the rule on an MI355X: the assertion of the rule on that plane,
        expected to fail.  The device run and everything else that could go wrong sits in the setup, outside what the mark accepts."""
        try:
            rows, _, _ = LX.compare_planes(LX.reference(name).rows, LX.oracle_view(name)[0], _lift_planes(lifter, name))
        except AssertionError as e:
            raise RuntimeError(f"setup of {name} failed: {e}") from e
        r = rows[LX.PLANES.index(plane)]
        print("  " + r.line())
        assert r.ok, r.line()
