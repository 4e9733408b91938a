"""The chain that turns status[] and cost[] into a winner and its counters -- block partials, rp_fold_partials_kernel,
rp_finalize_kernel / rp_select_kernel, the cost-ordered stage (rp_lazy_hist_kernel, rp_lazy_gather_kernel, list rounds), the bounded
sweep, rp_select and rp_count_collisions_before -- on the scenes of tests/_ladder.py: exact cost ties far apart in index, the
first free candidate in the first / second / third list, just behind the lists and beyond their capacity, over-full lists, "every
feasible candidate collides", "no feasible candidate", a cheapest cost of exactly 0.0; with option "fold_threshold" at its default
and at 4, on whole grids and on the shard [C/3, 2C/3).

Expected values: tests/_ladder.py: reference_selection (plain NumPy) applied to THE COSTS THE DEVICE RETURNED and THE ORACLE'S
LABELS, after the device costs have been held to the oracle's (1e-9 relative, equal NaN patterns) and the costs of duplicate
candidates to each other (equal as uint64) -- the selection is held exactly, a last-bit difference between two implementations of
the cost is not counted against it.  Mirror twins (-d / +d) are not required to be bit-equal on the device: whatever they are,
the selection over the device's costs is what is asserted (measured on an MI355X: all 2 664 twin pairs of both mirror scenes
bit-equal on each of the seven eager launch paths).

The cost-ordered stage says what it ran through option "lazy_trace" (one line per round on the library's stderr, read with
capfd); which candidates its lists hold is restated on the host (tests/_ladder.py: stage_model)."""
import functools
import re

import numpy as np
import pytest

import _ladder as LD
from _paths import LAUNCH_PATHS
from commonroad_rp_amd import _capi

pytestmark = pytest.mark.gpu

EAGER_PATHS = ("single_launch", "two_kernel", "g32", "g64", "wave_wg", "lane_cand", "lane_chunk")
EAGER_SCENES = tuple(n for n in sorted(LD.SCENES) if n not in (LD.LARGEST, LD.FOLD_ALIAS))     # the eager matrix: scenes up to ~48 000 candidates
STAGE_SCENES = tuple(n for n in sorted(LD.SCENES) if n != LD.FOLD_ALIAS)
# pass 1 of the cost-ordered stage / of the sweep by each of the three evaluation kernels
PASS1 = {
    "rp_eval_kernel": {"cost_kernel": 0, "chunk_kernel": 0},
    "rp_chunk_kernel": {"cost_kernel": 0, "chunk_kernel": 1},
    "rp_cost_kernel": {"cost_kernel": 1, "chunk_kernel": 0},
}
STAGE = {"fused_lon": 0, "lazy": 1, "auto_materialize": 0}
TRACE = re.compile(r"cost-ordered stage, round (\d+): list sizes (\d+) (\d+) (\d+), overflow bits ([0-9a-f]+), checked (\d+) of (\d+) feasible, winner (-?\d+)")


@pytest.fixture(scope="module")
def ctx():
    _capi.set_default_options(None)
    c = _capi.RpContext(0)
    yield c
    assert c.get_option("wait_fallbacks") == 0        # no chain of kernels ever failed to hand its completion ticket over
    c.close()
    _capi.set_default_options(None)


@pytest.fixture(autouse=True)
def _reset_options():
    yield
    _capi.set_default_options(None)


@functools.lru_cache(maxsize=None)
def _cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _ranges(name):
    C = LD.SCENES[name].n_candidates
    return ((0, C), (C // 3, 2 * C // 3))


def _variants(name):
    """(fold_threshold option or None, (lo, hi)): both fold settings on the whole grid and on the shard; the largest scene once"""
    if name == LD.LARGEST:
        return [(None, _ranges(name)[0])]
    return [(ft, r) for ft in (None, 4) for r in _ranges(name)]


def _plan(ctx, opts, ft, sc, lo, hi):
    o = dict(opts)
    if ft is not None:
        o["fold_threshold"] = ft
    _capi.set_default_options(o)
    sc.setup(ctx)
    out = ctx.plan(sc.inputs, lo, hi)
    status, cost = ctx.fetch_status()
    return out, status, cost


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _check_costs(sc, run, cost, lo, hi, what):
    """the device's costs against the oracle's: the project's contract (1e-9 relative), equal NaN patterns, duplicates bit-equal"""
    oc = run.cost[lo:hi]
    have = ~np.isnan(oc)
    assert np.array_equal(np.isnan(cost), ~have), what
    assert np.all(np.abs(cost[have] - oc[have]) <= 1e-9 * np.abs(oc[have])), (what, float(np.max(np.abs(cost[have] - oc[have]) / np.maximum(np.abs(oc[have]), 1e-300))))
    tid = sc.triple_ids()[lo:hi]
    order = np.argsort(tid, kind="stable")
    bits, t = cost.view(np.uint64)[order], tid[order]
    same = t[1:] == t[:-1]
    assert np.all(bits[1:][same] == bits[:-1][same]), what


def _check_result(out, cost, olab, ostatus, lo, what):
    """winner, best_cost bits, n_feasible, n_collision_before_best and the reason counters (n_collision depends on the path)"""
    wi, wc, nb = LD.reference_selection(cost, olab, lo)
    assert out.best_index == wi, (what, out.best_index, wi)
    if wi >= 0:
        assert _bits(out.best_cost) == _bits(wc), what
    else:
        assert np.isnan(out.best_cost), what
    assert out.n_candidates == len(cost), what
    assert out.n_feasible == np.count_nonzero((olab == 1) | (olab == 3)), what
    assert out.n_collision_before_best == nb, (what, out.n_collision_before_best, nb)
    np.testing.assert_array_equal(out.reason_counts, LD.reason_counts(ostatus), err_msg=str(what))
    return wi, wc, nb


def _ahead(cost, lo, wi, wc):
    """mask: candidates with a cost that sort before the winner (all of them without one)"""
    have = ~np.isnan(cost)
    if wi < 0:
        return have
    idx = lo + np.arange(len(cost))
    with np.errstate(invalid="ignore"):
        return have & ((cost < wc) | ((cost == wc) & (idx < wi)))


def _check_cost_ordered_labels(status, cost, ostatus, lo, wi, wc, what):
    """after a plan that answered the query in cost order: exact ahead of the winner (and on everything that has no cost);
    behind it the only difference is a colliding candidate nobody looked at"""
    lab, olab = status & 3, ostatus & 3
    ahead = _ahead(cost, lo, wi, wc) | np.isnan(cost)
    np.testing.assert_array_equal(status[ahead] & 0x7F, ostatus[ahead] & 0x7F, err_msg=str(what))
    diff = lab != olab
    assert np.all((olab[diff] == 3) & (lab[diff] == 1)), what


def test_both_epilogues_occur():
    sizes = [hi - lo for n in EAGER_SCENES for lo, hi in _ranges(n)]
    assert any(s > LD.SELECT_ABOVE for s in sizes) and any(0 < s <= LD.SELECT_ABOVE for s in sizes)   # rp_select_kernel / rp_finalize_kernel
    shards = [hi - lo for n in EAGER_SCENES if LD.SCENES[n].n_candidates > LD.SELECT_ABOVE for lo, hi in _ranges(n)[1:]]
    assert any(s <= LD.SELECT_ABOVE for s in shards)      # (and a shard of a large grid goes back to the one-workgroup epilogue)


@pytest.mark.parametrize("path", EAGER_PATHS)
@pytest.mark.parametrize("name", EAGER_SCENES)
def test_eager_selection(ctx, name, path):
    sc, run = LD.oracle_run(name)
    for ft, (lo, hi) in _variants(name):
        what = (name, path, ft, lo, hi)
        out, status, cost = _plan(ctx, dict(LAUNCH_PATHS[path], lazy=0), ft, sc, lo, hi)
        assert ctx.last_path() == 0, what
        ostatus = run.status[lo:hi]
        _check_costs(sc, run, cost, lo, hi, what)
        _check_result(out, cost, ostatus & 3, ostatus, lo, what)
        assert out.n_collision == np.count_nonzero((ostatus & 3) == 3), what
        np.testing.assert_array_equal(status & 0x7F, ostatus & 0x7F, err_msg=str(what))
    assert ctx.get_option("wait_fallbacks") == 0


@pytest.mark.parametrize("path", ["wave_wg", "g64", "two_kernel"])
def test_fold_keeps_the_lowest_index_of_a_tie(ctx, path):
    """131 072 candidates, four per workgroup on wave_wg and g64 (32 768 block partials: folded at the default threshold too): the
    partial of the winner and the partial of a free copy of it, 65 536 candidates on, are reduced by the same lane of
    rp_fold_partials_kernel -- the one level of the chain where two tied partials meet in a plain loop"""
    name = LD.FOLD_ALIAS
    sc, run = LD.oracle_run(name)
    C = sc.n_candidates
    for ft in (None, 4):
        what = (name, path, ft)
        out, status, cost = _plan(ctx, dict(LAUNCH_PATHS[path], lazy=0), ft, sc, 0, C)
        assert ctx.last_path() == 0, what
        _check_costs(sc, run, cost, 0, C, what)
        _check_result(out, cost, run.status & 3, run.status, 0, what)
        assert out.n_collision == run.out.n_collision, what
        np.testing.assert_array_equal(status & 0x7F, run.status & 0x7F, err_msg=str(what))


@pytest.mark.parametrize("name", ["mirror_rank721", "mirror_rank73", "rank1584", "g48_rank12000"])
def test_count_collisions_before_inside_tie_groups(ctx, name):
    sc, run = LD.oracle_run(name)
    for ft, (lo, hi) in _variants(name):
        out, status, cost = _plan(ctx, dict(LAUNCH_PATHS["two_kernel"], lazy=0), ft, sc, lo, hi)
        lab = status & 3
        np.testing.assert_array_equal(lab, run.status[lo:hi] & 3)
        groups = [g for g in LD.tie_groups(cost, lab) if len(g) >= 3 and np.any(lab[g] == 3)]
        assert len(groups) >= 3, name
        for g in (groups[0], groups[len(groups) // 2], groups[-1]):
            c = float(cost[g[0]])
            for idx in (g[0], g[0] + 1, g[len(g) // 2], g[-1], g[-1] + 1):
                key = lo + int(idx)
                assert ctx.count_collisions_before(c, key) == LD.count_before(cost, lab, c, key, lo), (name, ft, lo, c, key)


@pytest.mark.parametrize("name", ["g48_rank10080", "g48_rank24080", "all_collide_24880"])
def test_select_with_caller_costs_full_of_ties(ctx, name):
    sc, run = LD.oracle_run(name)
    C = sc.n_candidates
    assert C > LD.SELECT_ABOVE
    for ft in (None, 4):
        out, status, cost = _plan(ctx, dict(LAUNCH_PATHS["two_kernel"], lazy=0), ft, sc, 0, C)
        assert ctx.last_path() == 0
        lab = status & 3
        np.testing.assert_array_equal(lab, run.status & 3)
        third = cost.copy()
        third[np.arange(C) % 3 == 1] = np.nan
        for tag, user in (("all equal", np.ones(C)), ("floor", np.floor(cost)), ("NaN on a third", third)):
            eff = np.where((lab == 1) | (lab == 3), user, np.nan)       # (candidates without a cost of their own do not take one)
            wi, wc, nb = LD.reference_selection(eff, lab)
            got = ctx.select(user)
            assert got.best_index == wi, (name, ft, tag, got.best_index, wi)
            assert np.isnan(got.best_cost) if wi < 0 else _bits(got.best_cost) == _bits(wc), (name, ft, tag)
            assert got.n_collision_before_best == nb, (name, ft, tag, got.n_collision_before_best, nb)
            assert got.n_feasible == run.out.n_feasible and got.n_collision == run.out.n_collision


@pytest.mark.parametrize("kernel", sorted(PASS1))
@pytest.mark.parametrize("name", STAGE_SCENES)
def test_cost_ordered_stage_list_rounds(ctx, capfd, name, kernel):
    sc, run = LD.oracle_run(name)
    seen_paths = set()
    for ft, (lo, hi) in _variants(name):
        what = (name, kernel, ft, lo, hi)
        capfd.readouterr()
        out, status, cost = _plan(ctx, dict(STAGE, lazy_trace=1, **PASS1[kernel]), ft, sc, lo, hi)
        trace = [tuple(int(v, 16) if k == 4 else int(v) for k, v in enumerate(m.groups())) for m in TRACE.finditer(capfd.readouterr().err)]
        assert ctx.last_kernel() == kernel, what
        ostatus = run.status[lo:hi]
        olab = ostatus & 3
        _check_costs(sc, run, cost, lo, hi, what)
        wi, wc, nb = _check_result(out, cost, olab, ostatus, lo, what)
        sm = LD.stage_model(cost, olab, lo)
        count = hi - lo
        sweeps = count > LD.SELECT_ABOVE and count >= LD.SWEEP_MIN_PER_CU * _cu_count()
        want_path = 1 if sm.path == 1 else (3 if sweeps else 2)
        assert ctx.last_path() == want_path, (what, ctx.last_path(), want_path, sm.sizes, sm.overflow, trace)
        seen_paths.add(want_path)
        lab = status & 3
        # the trace: one line per round that ran, each with the list sizes and overflow bits the histogram fixed
        assert tuple(t[0] for t in trace) == sm.ran, (what, trace, sm)
        for t in trace:
            assert t[1:4] == sm.sizes and t[4] == sm.overflow and t[6] == sm.n_feasible, (what, t, sm)
        if want_path == 1:
            assert sm.winner == wi, what
            m = sum(trace[-1][1 + t[0]] for t in trace)
            order = LD.sort_order(cost)
            # the lists are prefixes of the cost order that reach their targets and end between tie groups
            cum = np.cumsum(trace[-1][1:4])
            ends = np.cumsum([len(g) for g in LD.tie_groups(cost, olab)]) if sm.n_feasible else np.zeros(0)
            for l in range(3):
                assert cum[l] >= min(LD.LIST_TARGET[l], sm.n_feasible) and (cum[l] == 0 or cum[l] in ends), (what, trace)
            assert m == 0 or m in ends, (what, m)
            # the rounds stop at the first prefix that holds a free candidate (or once every feasible candidate has been looked at)
            ran = [t[0] for t in trace]
            for l in ran[:-1]:
                assert not np.any(olab[order[:cum[l]]] == 1), (what, l)
            assert np.any(olab[order[:cum[ran[-1]]]] == 1) if wi >= 0 else m >= sm.n_feasible, what
            # labelled = exactly the oracle's colliding candidates among the first m of the cost order
            want3 = np.sort(order[:m][olab[order[:m]] == 3])
            np.testing.assert_array_equal(np.flatnonzero(lab == 3), want3, err_msg=str(what))
            np.testing.assert_array_equal(want3, np.sort(sm.labelled))
            assert out.n_collision == len(want3), what
            other = lab != 3
            np.testing.assert_array_equal(status[other] & 0x7F, np.where(olab[other] == 3, 1, ostatus[other] & 0x7F), err_msg=str(what))
        elif want_path == 2:   # the eager kernel decided: every label
            np.testing.assert_array_equal(status & 0x7F, ostatus & 0x7F, err_msg=str(what))
            assert out.n_collision == np.count_nonzero(olab == 3), what
        else:                  # exhausted lists handed over to the sweep
            _check_cost_ordered_labels(status, cost, ostatus, lo, wi, wc, what)
            assert out.n_collision == out.n_collision_before_best, what
    if name == LD.LARGEST:
        assert seen_paths == {3 if LD.SCENES[name].n_candidates >= LD.SWEEP_MIN_PER_CU * _cu_count() else 2}
    assert ctx.get_option("wait_fallbacks") == 0


@pytest.mark.parametrize("kernel", sorted(PASS1))
@pytest.mark.parametrize("name", STAGE_SCENES)
def test_bounded_sweep(ctx, name, kernel):
    sc, run = LD.oracle_run(name)
    for ft, (lo, hi) in _variants(name):
        what = (name, kernel, ft, lo, hi)
        out, status, cost = _plan(ctx, dict(STAGE, sweep=1, **PASS1[kernel]), ft, sc, lo, hi)
        assert ctx.last_path() == 3 and ctx.last_kernel() == kernel, (what, ctx.last_path(), ctx.last_kernel())
        ostatus = run.status[lo:hi]
        _check_costs(sc, run, cost, lo, hi, what)
        wi, wc, nb = _check_result(out, cost, ostatus & 3, ostatus, lo, what)
        assert out.n_collision == out.n_collision_before_best, what
        _check_cost_ordered_labels(status, cost, ostatus, lo, wi, wc, what)
    assert ctx.get_option("wait_fallbacks") == 0
