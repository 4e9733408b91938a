"""The scene table of tests/_ladder.py covers the cases tests/test_selection_edges.py is about -- asserted on the CPU oracle alone.
These are conditions on the scenes, not measurements: a scene that stops meeting one is retuned (wall width / offset / distance,
grid sizes), the condition stays.

Two groups of bit-equal costs are NOT duplicates of one (T, L, D) triple, both by construction:
  * the mirror scenes: candidates at -d and +d tie (that is what they are for) -- their groups are duplicates of one (T, L, |D|);
  * the zero-cost group of `zero_cost`: L = 10 and D = 0 keep the initial state for any duration, so both T values cost exactly 0.0
    (a cost of zero and groups that never mix durations exclude each other on a grid that alternates two durations)."""
import numpy as np
import pytest

import _ladder as LD

ALL = sorted(LD.SCENES)


def _facts(name):
    sc, run = LD.oracle_run(name)
    lab = run.status & 3
    return sc, run, lab, LD.tie_groups(run.cost, lab)


def _rank(name):
    _, run, lab, _ = _facts(name)
    return LD.rank_of_winner(run.cost, lab)


def _winner_group(name):
    _, run, lab, groups = _facts(name)
    wi = run.out.best_index
    return next(g for g in groups if wi in g)


@pytest.mark.parametrize("name", ALL)
def test_reference_selection_is_the_oracles(name):
    sc, run, lab, _ = _facts(name)
    wi, wc, nb = LD.reference_selection(run.cost, lab)
    assert (wi, nb) == (run.out.best_index, run.out.n_collision_before_best)
    assert wi < 0 or wc == run.out.best_cost
    assert run.out.n_feasible == np.count_nonzero((lab == 1) | (lab == 3)) and run.out.n_collision == np.count_nonzero(lab == 3)
    np.testing.assert_array_equal(LD.reason_counts(run.status), run.out.reason_counts)
    assert np.array_equal(np.isnan(run.cost), (lab != 1) & (lab != 3))
    assert len(sc.obstacles.static_obb) == 1                       # (every scene keeps its wall)


@pytest.mark.parametrize("name", ALL)
def test_no_near_ties_and_ties_are_duplicates(name):
    sc, run, lab, groups = _facts(name)
    if not groups:
        return
    gc = np.array([run.cost[g[0]] for g in groups])
    assert np.all(np.diff(gc) > 1e-6 * np.maximum(1.0, np.abs(gc[1:]))), name
    tid = sc.triple_ids()
    sp = sc.spec
    for g in groups:
        ids = np.unique(tid[g])
        if len(ids) == 1:
            continue
        iT, iL, iD = ids // (sp.nLu * sp.nDu), (ids // sp.nDu) % sp.nLu, ids % sp.nDu
        if name in LD.MIRROR:          # one (T, L) and the two lateral samples -d, +d
            assert len(ids) == 2 and iT[0] == iT[1] and iL[0] == iL[1] and iD[0] + iD[1] == sp.nDu - 1, (name, ids)
        else:                          # the zero-cost group: one (L, D) = (10, 0), both durations
            assert name == "zero_cost" and run.cost[g[0]] == 0.0 and len(ids) == 2 and iL[0] == iL[1] and iD[0] == iD[1], (name, ids)
            assert sc.inputs.L[iL[0]] == 10.0 and sc.inputs.D[iD[0]] == 0.0
    # duplicates tie: every triple's copies carry one cost (or none)
    order = np.argsort(tid, kind="stable")
    bits = run.cost.view(np.uint64)[order]
    same = tid[order][1:] == tid[order][:-1]
    assert np.all(bits[1:][same] == bits[:-1][same])


def test_winner_ranks_cover_the_lists_and_beyond():
    ranks = {n: _rank(n) for n in ALL}
    C = {n: LD.SCENES[n].n_candidates for n in ALL}

    def some(lo, hi, cond=lambda n: True):
        return [n for n in ALL if ranks[n] is not None and lo <= ranks[n] <= hi and cond(n)]
    zero = some(0, 0, lambda n: np.ptp(_winner_group(n)) >= 4096)
    assert zero, ranks
    assert some(1, 127) and some(128, 1023) and some(1024, 8191) and some(8192, 16383), ranks
    assert some(LD.LIST_TOTAL + 1, 10 ** 9, lambda n: C[n] < 131072), ranks
    assert some(LD.LIST_TOTAL + 1, 10 ** 9, lambda n: C[n] >= 134000), ranks
    assert ranks[LD.LARGEST] > LD.LIST_TOTAL and C[LD.LARGEST] >= 134000


def test_every_feasible_candidate_collides_at_three_sizes():
    sizes = []
    for n in ALL:
        _, run, lab, _ = _facts(n)
        if run.out.n_feasible > 0 and run.out.best_index < 0:
            assert run.out.n_collision == run.out.n_feasible == run.out.n_collision_before_best
            sizes.append(run.out.n_feasible)
    assert any(s < 128 for s in sizes) and any(1024 <= s <= 8191 for s in sizes) and any(s > LD.LIST_TOTAL for s in sizes), sizes


def test_no_feasible_candidate_and_zero_cost():
    _, run, lab, _ = _facts("none_feasible")
    assert run.out.n_feasible == 0 and run.out.best_index == -1 and not np.any((lab == 1) | (lab == 3))
    _, run, lab, groups = _facts("zero_cost")
    assert run.cost[groups[0][0]] == 0.0 and np.signbit(run.cost[groups[0][0]]) == False and run.out.best_index >= 0   # noqa: E712


def test_overflow_scenes():
    _, run, lab, groups = _facts("overflow_free")
    assert len(groups[0]) > LD.LIST_CAP[0] and np.all(lab[groups[0]] == 1) and run.out.best_index == groups[0][0]
    _, run, lab, groups = _facts("overflow_blocked")
    assert len(groups[0]) > LD.LIST_CAP[0] and np.all(lab[groups[0]] == 3)
    assert run.out.best_index >= 0 and run.out.best_index not in groups[0] and run.out.n_collision_before_best >= len(groups[0])
    for n in ("overflow_free", "overflow_blocked"):
        _, run, lab, _ = _facts(n)
        sm = LD.stage_model(run.cost, lab)
        assert sm.overflow & 1 and sm.path == 2 and sm.ran == (0,)


@pytest.mark.parametrize("name", LD.MIRROR)
def test_mirror_scene_mixes_free_and_colliding_twins(name):
    _, run, lab, _ = _facts(name)
    g = _winner_group(name)
    wi = run.out.best_index
    assert np.any(lab[g] == 1) and np.any(lab[g] == 3)
    assert np.any((lab[g] == 3) & (g < wi)) and np.any((lab[g] == 3) & (g > wi))


def test_ties_span_select_slices_and_fold_slots():
    """in at least three scenes beyond the one-workgroup epilogue the winner's tie group falls into three or more 2 048-candidate
    slices of rp_select_kernel and into workgroups whose partials land in different slots after a fold to 256 (partial k goes to slot
    (k mod 16 384) div 64: rp_fold_partials_kernel) -- for every number of candidates per workgroup the evaluation kernels have"""
    good = []
    for n in ALL:
        _, run, lab, _ = _facts(n)
        if LD.SCENES[n].n_candidates <= LD.SELECT_ABOVE or run.out.best_index < 0:
            continue
        g = _winner_group(n)
        slices = len(np.unique(g // LD.SEL_SLICE))
        slots = min(len(np.unique(((g // per_wg) % (LD.FOLD_SLOTS * 64)) // 64)) for per_wg in (4, 8, 16, 64))
        if slices >= 3 and slots >= 2:
            good.append(n)
    assert len(good) >= 3, good


def test_stage_model_reaches_every_exit():
    """what the host-side restatement of the cost-ordered stage says about the table: a winner in each of the three lists, the
    "every feasible candidate collides" exits of rounds 0 and 2, "no feasible candidate", overflow, lists exhausted below and at
    the sweep's size -- and its lists are cost prefixes that reach their targets without splitting a tie group"""
    seen = set()
    for n in ALL:
        sc, run, lab, groups = _facts(n)
        sm = LD.stage_model(run.cost, lab)
        won = sm.winner is not None and sm.winner >= 0
        seen.add((sm.path, len(sm.ran), won, bool(sm.overflow), sm.n_feasible == 0, LD.SCENES[n].n_candidates >= 131072))
        if sm.path == 1:
            assert sm.winner == run.out.best_index, n
        if not sm.overflow and sm.n_feasible:
            cum = np.cumsum(sm.sizes)
            ends = np.cumsum([len(g) for g in groups])
            for l in range(3):
                assert cum[l] >= min(LD.LIST_TARGET[l], sm.n_feasible) and cum[l] in ends, (n, sm.sizes)
    F = False
    for want in ((1, 1, True, F, F, F), (1, 2, True, F, F, F), (1, 3, True, F, F, F), (1, 1, F, F, F, F), (1, 3, F, F, F, F), (1, 1, F, F, True, F),
                 (2, 1, F, True, F, F), (2, 3, F, F, F, F), (2, 3, F, F, F, True)):
        assert want in seen, (want, sorted(seen))


def test_fold_alias_scene():
    """the winner and a free copy of it in partials 16 384 apart at four candidates per workgroup: one lane of the fold sees both"""
    _, run, lab, _ = _facts(LD.FOLD_ALIAS)
    g = _winner_group(LD.FOLD_ALIAS)
    wi = run.out.best_index
    k = g // 4
    twins = g[(k != wi // 4) & ((k - wi // 4) % (LD.FOLD_SLOTS * 64) == 0)]
    assert wi == g[0] and len(twins) >= 1 and np.all(lab[twins] == 1)
    assert LD.SCENES[LD.FOLD_ALIAS].n_candidates // 4 > 8192      # (folds at the default threshold too)
