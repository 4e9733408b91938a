"""The host twin of the winner exchange -- commonroad_rp_amd.distributed.pack_result / combine_results, what the gloo and the
host-packed transports run -- on partitions that put exact cost ties, ranks without a free / a feasible candidate and empty ranks in
front of it.  Oracle only: every range of a partition (tests/_shards.py) is planned by the oracle on its own, packed and combined,
and the result is held to tests/_ladder.py: reference_selection over the UNSHARDED oracle run: winner, best_cost bits, owner rank,
summed counters, the owner's rows and coefficients (bit-equal to the unsharded winner's: the oracle evaluates a candidate the same
way in every range) and the second message -- colliding candidates that sort before the global winner, restated with NumPy on each
shard's own arrays and summed.

The table assertions below are conditions on the scenes and cuts, as in tests/test_ladder_scenes.py: a partition that stops meeting one
is retuned, the condition stays."""
import functools

import numpy as np
import pytest

import _ladder as LD
import _shards as SH
from commonroad_rp_amd.distributed import combine_results, pack_result

SCENES = SH.SMALL_SCENES + (LD.N40,)


@functools.lru_cache(maxsize=None)
def _tables(name):
    sc, _ = LD.oracle_run(name)
    return sc.oracle_tables()


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _combine(name, ranges):
    """(global result, owner, per-rank oracle runs) of the partition"""
    from oracle import oracle
    sc, _ = LD.oracle_run(name)
    n = sc.inputs.params.N + 1
    runs = [oracle.plan(sc.inputs, _tables(name), lo, hi, want_states=False, nthreads=2 if hi - lo > 2048 else 1) for lo, hi in ranges]
    msgs = np.stack([pack_result(r.out, n) for r in runs])
    glob, owner = combine_results(msgs, n)
    return glob, owner, runs


def test_scene_list():
    assert len(SH.SMALL_SCENES) >= 12 and all(LD.SCENES[n].n_candidates <= 10000 for n in SH.SMALL_SCENES)
    assert set(LD.MIRROR) <= set(SH.SMALL_SCENES) and "none_feasible" in SH.SMALL_SCENES and "all_collide_4248" in SH.SMALL_SCENES
    sc, run = LD.oracle_run(LD.N40)
    assert sc.inputs.params.N == 40 and run.out.best_index >= 0 and run.out.n_collision_before_best > 0
    assert all(LD.SCENES[n].n_steps == 20 for n in LD.SCENES)


def test_partitions_cover_what_the_combine_step_can_get_wrong():
    seen = {}
    for name in SCENES:
        sc, run = LD.oracle_run(name)
        lab = run.status & 3
        for tag, ranges in SH.partitions(name, SH.HOST_WORLDS):
            SH.check_partition(ranges, sc.n_candidates)
            for f in SH.facts(run.cost, lab, ranges):
                seen.setdefault(f, []).append((name, tag))
    for f in SH.WANTED:
        assert seen.get(f), (f, sorted(seen))
    # the cut behind the first copy of the cheapest tie group really leaves that copy alone with its twins on the other side
    for name in ("rank0_far_ties", "overflow_free", "mirror_rank73"):
        sc, run = LD.oracle_run(name)
        g = LD.tie_groups(run.cost, run.status & 3)[0]
        (lo0, hi0), (lo1, hi1) = SH.explicit_cuts(name)["behind_first_copy"]
        assert hi0 == g[0] + 1 and len(g) >= 2 and np.all(g[1:] >= lo1)
    # a free winner whose bit-equal copies sit in a LATER rank (a combine step that lets the later of two equal costs win moves it)
    # and one with a colliding copy in an EARLIER rank (a collisions-before count that forgets the index order loses it)
    later = earlier = 0
    for name in SCENES:
        sc, run = LD.oracle_run(name)
        lab = run.status & 3
        wi = run.out.best_index
        if wi < 0:
            continue
        g = next(g for g in LD.tie_groups(run.cost, lab) if wi in g)
        for tag, ranges in SH.partitions(name, SH.HOST_WORLDS):
            own = SH.rank_of(ranges, wi)
            later += any(lab[i] == 1 and SH.rank_of(ranges, i) > own for i in g)
            earlier += any(lab[i] == 3 and SH.rank_of(ranges, i) < own for i in g)
    assert later >= 10 and earlier >= 4, (later, earlier)


@pytest.mark.parametrize("name", SCENES)
def test_packed_and_combined_shards_equal_the_unsharded_selection(name):
    sc, run = LD.oracle_run(name)
    lab = run.status & 3
    wi, wc, nb = LD.reference_selection(run.cost, lab)
    assert (wi, nb) == (run.out.best_index, run.out.n_collision_before_best)
    for tag, ranges in SH.partitions(name, SH.HOST_WORLDS):
        what = (name, tag)
        glob, owner, runs = _combine(name, ranges)
        assert glob.best_index == wi, (what, glob.best_index, wi)
        assert owner == SH.rank_of(ranges, wi), (what, owner)
        if wi >= 0:
            assert _bits(glob.best_cost) == _bits(wc), what
            np.testing.assert_array_equal(glob.best_states, runs[owner].out.best_states, err_msg=str(what))
            np.testing.assert_array_equal(glob.best_states, run.out.best_states, err_msg=str(what))
            np.testing.assert_array_equal(glob.best_lon_coeffs, run.out.best_lon_coeffs, err_msg=str(what))
            np.testing.assert_array_equal(glob.best_lat_coeffs, run.out.best_lat_coeffs, err_msg=str(what))
            assert glob.best_lat_T == run.out.best_lat_T, what
        else:
            assert owner == -1 and np.isnan(glob.best_cost) and glob.best_states is None, what
        assert (glob.n_candidates, glob.n_feasible, glob.n_collision) == (run.out.n_candidates, run.out.n_feasible, run.out.n_collision), what
        np.testing.assert_array_equal(glob.reason_counts, run.out.reason_counts, err_msg=str(what))
        # every shard is the slice of the unsharded run (costs as bits), so the restated second message is over the same numbers
        total = 0
        for (lo, hi), r in zip(ranges, runs):
            np.testing.assert_array_equal(r.cost.view(np.uint64), run.cost[lo:hi].view(np.uint64), err_msg=str(what))
            np.testing.assert_array_equal(r.status, run.status[lo:hi], err_msg=str(what))
            slab = r.status & 3
            if glob.best_index < 0:
                total += int(np.count_nonzero(slab == 3))
            else:
                total += LD.count_before(r.cost, slab, glob.best_cost, glob.best_index, lo)
        assert total == nb, (what, total, nb)


@pytest.mark.parametrize("name", ["rank0_far_ties", "rank936", "mirror_rank73", "all_collide_4248", "none_feasible"])
def test_equal_messages_belong_to_the_first_rank(name):
    """two ranks that planned the same range send messages equal in (cost, index): the owner is the FIRST of them (every rank must
    name the same owner -- it alone reports its own collisions-before count -- and rp_combine_kernel keeps the first as well)"""
    sc, run = LD.oracle_run(name)
    wi, wc, _ = LD.reference_selection(run.cost, run.status & 3)
    for tag, ranges in SH.replicated(name):
        glob, owner, runs = _combine(name, ranges)
        assert glob.best_index == wi and owner == (0 if wi >= 0 else -1), (name, tag, glob.best_index, owner)
        assert np.isnan(glob.best_cost) if wi < 0 else _bits(glob.best_cost) == _bits(wc), (name, tag)
        assert (glob.n_candidates, glob.n_feasible, glob.n_collision) == (2 * run.out.n_candidates, 2 * run.out.n_feasible, 2 * run.out.n_collision)
        np.testing.assert_array_equal(glob.reason_counts, 2 * run.out.reason_counts)
