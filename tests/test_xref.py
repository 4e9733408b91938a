"""The evaluation kernels against the extended-precision reference of tests/_xref.py: state rows, costs, the winner's rows and
coefficients, and the explicit-polynomial tier that separates the solve from the evaluation.  Needs a real MI355X: ``pytest -m gpu``.

No tolerance here is taken from the device: a device row may be MARGIN_MAX = 8 times as far from the reference as the double oracle's
row is, plus 8 spacings of the row's scale, and 4 times in the root mean square plus 2 spacings (the rule and its reasons:
tests/_xref.py); what the oracle's own distance is, and that the comparison fails on planted defects, tests/test_xref_abi.py checks
without a GPU.  Every test prints E_O, E_D and their ratio per row; `python tests/_xref.py` writes them to profiles/accuracy_xref.txt."""
import numpy as np
import pytest

import _xref as XR
from _bitid import chunk_applies
from _paths import LAUNCH_PATHS
from commonroad_rp_amd._capi import RpContext, FLAG_MATERIALIZE_ALL
from commonroad_rp_amd.collision import ObstacleTables

WINNER_PASS = {"fused_lon": 0, "auto_materialize": 0}   # two-kernel path that stores no rows: the winner's come from the re-evaluation pass

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not XR.HAVE_LONGDOUBLE, reason=XR.SKIP_REASON)]


@pytest.fixture(scope="module")
def contexts():
    """one context per launch path (and per launch variant that stores rows), made when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            ctx = RpContext(0)
            opts = XR.STATE_VARIANTS[name] if name in XR.STATE_VARIANTS else (WINNER_PASS if name == "winner_pass" else LAUNCH_PATHS[name])
            for k, v in opts.items():
                ctx.set_option(k, v)
            made[name] = ctx
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


KNOWN = XR.KNOWN_EXCEEDANCES   # (tier, case, row) -> diagnosis: asserted on their own, expected to fail (test_known_exceedance)


def _assert_rows(tier, name, rows):
    """every row within the rule, except the known exceedances of this tier and case: those are asserted by test_known_exceedance"""
    found = [r.line() for r in rows if not r.ok and (tier, name, r.row) not in KNOWN]
    assert not found, "\n".join([f"{name} ({tier}):"] + found)


def _setup(ctx, name):
    c = XR.case(name)
    ctx.set_coordinate_system(c.co)
    ctx.set_obstacles(ObstacleTables())
    return c


def _report(what, rows, n_out):
    print(f"{what} ({n_out} candidates left out)")
    for r in rows:
        print("  " + r.line())


@pytest.mark.parametrize("name", XR.CASE_NAMES)
@pytest.mark.parametrize("variant", list(XR.STATE_VARIANTS))
def test_state_rows(contexts, variant, name):
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    got, launch = XR.device_rows(contexts(variant), name, variant)   # (asserts that what the variant's options force is what ran)
    rows, n_out = XR.compare_rows(ref.states, states, got, mask)
    _report(f"{name} on {variant} {launch}", rows, n_out)
    assert not XR.failures(rows), "\n".join([f"{name} on {variant}:"] + XR.failures(rows))


def test_variants_reach_every_kernel_instance(contexts):
    """between them the variants and cases run rp_eval_kernel with 16, 32 and 64 lanes, in one launch and in two, and the fixed-stride
    (lean step block) variant as well as the generic one"""
    ran = {XR.device_rows(contexts(v), name, v)[1][1:] for v in XR.STATE_VARIANTS for name in XR.CASE_NAMES}
    assert ran >= XR.KERNEL_INSTANCES, XR.KERNEL_INSTANCES - ran


def _cost_kernel(path, N):
    """the kernel a production-mode plan without a collision query takes on a launch path (tests/_paths.py)"""
    if path == "lane_cand":
        return "rp_cost_kernel"
    if path == "lane_chunk" and chunk_applies(N):   # (rp_chunk_kernel serves 17 .. 112 steps)
        return "rp_chunk_kernel"
    return "rp_eval_kernel"


@pytest.mark.parametrize("name", XR.CASE_NAMES)
@pytest.mark.parametrize("path", list(LAUNCH_PATHS))
def test_costs(contexts, path, name):
    ctx = contexts(path)
    c = _setup(ctx, name)
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    ctx.plan(XR.production(c.inp))
    assert ctx.last_kernel() == _cost_kernel(path, c.inp.params.N), (path, ctx.last_kernel())
    if "lanes" in LAUNCH_PATHS[path] and ctx.last_kernel() == "rp_eval_kernel":
        assert ctx.get_option("last_lanes") == LAUNCH_PATHS[path]["lanes"]
    if LAUNCH_PATHS[path].get("fused_lon", 1) == 0:
        assert ctx.get_option("last_single_launch") == 0
    st, cs = ctx.fetch_status()
    feasible = ((status & 3) == 1) & XR.production_feasible(name)
    assert ((st[ref.index] & 3) == 1)[feasible].all()   # (labels are compared exactly elsewhere; here: the costs exist)
    sel = feasible & ~XR.left_out(ref.states, states, mask)
    e_o, e_d, bound = XR.compare_costs(ref.cost, cost, cs[ref.index], sel, c.inp.params.N)
    print(f"{name} costs on {path} ({ctx.last_kernel()}): oracle {e_o:.3e} device {e_d:.3e} bound {bound:.3e} relative, {int(sel.sum())} candidates")
    assert sel.any() and e_d <= bound


def _winner_plan(contexts, name):
    """a production-mode plan on the two-kernel path that stores no rows: the winner's rows come from the re-evaluation pass"""
    ctx = contexts("winner_pass")
    c = _setup(ctx, name)
    out = ctx.plan(XR.production(c.inp))
    assert ctx.get_option("last_single_launch") == 0 and out.best_index >= 0 and out.best_states is not None
    return ctx, c, out


def _winner_rows(contexts, name):
    ctx, c, out = _winner_plan(contexts, name)
    all_status, _, _, all_states = XR.oracle_run(name)
    w = int(out.best_index)
    assert (all_status[w] & 3) == 1
    rw = XR.reference_for(name, (w,))
    rows, n_out = XR.compare_rows(rw.states, all_states[w:w + 1], out.best_states[None], np.ones((1, c.inp.params.N + 1), dtype=bool))
    assert n_out == 0
    return w, rows


def _single_rows(contexts, name):
    """rp_eval_one of the first, the middle and the last feasible candidate of the case's subset, compared as ONE set of elements
    (candidate x step), as the rule is defined; their labels are asserted here"""
    ctx, c, out = _winner_plan(contexts, name)
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    js = XR.single_candidates(name)
    ones = []
    for j in js:
        one, st1, c1 = ctx.eval_one(int(ref.index[j]))
        assert (st1 & 3) == 1, (name, int(ref.index[j]), hex(st1))
        ones.append(one)
    rows, n_out = XR.compare_rows(ref.states[js], states[js], np.stack(ones), np.ones((3, c.inp.params.N + 1), dtype=bool))
    assert n_out == 0
    return [int(ref.index[j]) for j in js], rows


def _explicit_rows(contexts, variant, name):
    ctx = contexts(variant)
    c = _setup(ctx, name)
    lon, lat, T, tl, ref, status, cost, states = XR.coeffs_tier(name)
    p = XR.with_flags(c.inp, set_=FLAG_MATERIALIZE_ALL).params
    ctx.plan_coeffs(p, c.inp.cost, lon, lat, T, tl)
    found = XR.forced_launch_differences(XR.STATE_VARIANTS[variant], XR.launch_of(ctx))
    assert not found, (variant, XR.launch_of(ctx), found)
    mask = XR.compared_steps(status, p.N + 1, c.spec.draw)
    rows, n_out = XR.compare_rows(ref.states, states, ctx.fetch_states(), mask)
    return ctx, rows, n_out, mask


@pytest.mark.parametrize("name", XR.CASE_NAMES)
def test_winner_rows(contexts, name):
    w, rows = _winner_rows(contexts, name)
    _report(f"{name}: best_states of candidate {w}", rows, 0)
    _assert_rows("winner", name, rows)


@pytest.mark.parametrize("name", XR.CASE_NAMES)
def test_winner_coefficients(contexts, name):
    """best_lon_coeffs / best_lat_coeffs against the reference's: 8 times the oracle's distance (rpo_quintic_coeffs, rpo_quartic_coeffs:
    pivoted elimination) plus 8 spacings, per coefficient"""
    ctx, c, out = _winner_plan(contexts, name)
    w = int(out.best_index)
    rw = XR.reference_for(name, (w,))
    all_coeffs = XR.oracle_run(name)[2]
    for which, cX, cO, cD in (("lon", rw.lon[0], all_coeffs[w, :6], out.best_lon_coeffs), ("lat", rw.lat[0], all_coeffs[w, 6:12], out.best_lat_coeffs)):
        e_o, e_d, ok = XR.compare_coeffs(cX, cO, cD)
        print(f"{name}: {which} coefficients of the winner {w}: oracle {e_o} device {e_d}")
        assert ok, (which, e_o, e_d)


@pytest.mark.parametrize("name", XR.CASE_NAMES)
def test_single_candidates(contexts, name):
    cands, rows = _single_rows(contexts, name)
    _report(f"{name}: rp_eval_one of the candidates {cands}", rows, 0)
    _assert_rows("single", name, rows)


EXPLICIT_VARIANTS = ("default", "two_kernel_16")


@pytest.mark.parametrize("name", XR.CASE_NAMES)
@pytest.mark.parametrize("variant", EXPLICIT_VARIANTS)
def test_explicit_polynomials(contexts, variant, name):
    """rp_plan_coeffs fed the reference's coefficients, rounded to double: device, oracle and reference evaluate the SAME polynomials --
    a finding here sits in the evaluation, one that shows only in test_state_rows in the solve"""
    ctx, rows, n_out, mask = _explicit_rows(contexts, variant, name)
    c = XR.case(name)
    lon, lat, T, tl, ref, status, cost, states = XR.coeffs_tier(name)
    _report(f"{name}: explicit polynomials on {variant} {XR.launch_of(ctx)}", rows, n_out)
    _assert_rows("explicit", name, rows)
    st, cs = ctx.fetch_status()
    sel = ((status & 3) == 1) & ~XR.left_out(ref.states, states, mask)
    e_o, e_d, bound = XR.compare_costs(ref.cost, cost, cs, sel, c.inp.params.N)
    print(f"{name}: costs of explicit polynomials on {variant}: oracle {e_o:.3e} device {e_d:.3e} bound {bound:.3e}")
    assert e_d <= bound


_KNOWN_PARAMS = [(tier, name, row, variant) for (tier, name, row) in KNOWN for variant in (EXPLICIT_VARIANTS if tier == "explicit" else ("",))]


@pytest.mark.parametrize("tier,name,row,variant", [pytest.param(*k, marks=pytest.mark.xfail(strict=True, raises=AssertionError, reason=KNOWN[k[:3]]),
                                                                id="-".join(x for x in k if x)) for k in _KNOWN_PARAMS])
def test_known_exceedance(contexts, tier, name, row, variant):
    """ONE row of one comparison that exceeds the rule on an MI355X: the assertion of the rule on that row, expected to fail.  The device
    runs and everything else that could go wrong sits in the setup, outside what the mark accepts."""
    try:
        rows = {"winner": lambda: _winner_rows(contexts, name)[1], "single": lambda: _single_rows(contexts, name)[1],
                "explicit": lambda: _explicit_rows(contexts, variant, name)[1]}[tier]()
    except AssertionError as e:   # (an assertion of the setup is not the expected failure)
        raise RuntimeError(f"setup of {tier} {name} failed: {e}") from e
    r = rows[XR.ROWS.index(row)]
    print("  " + r.line())
    assert r.ok, r.line()
