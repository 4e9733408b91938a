"""Sharded plans against the unsharded plan on exact ties, on the device.

One context plays every rank in turn: shard r is planned, its device result block (rp_result_device) is copied into row r of ONE message
tensor with a device copy -- what all_gather_into_tensor leaves on every rank --, then rp_combine_kernel (rp_combine_results) runs on it,
once with the context holding the last rank's plan and once holding rank 0's; for the second message every shard is planned again and
distributed.local_collisions_before is summed.  Partitions: tests/_shards.py (shard_range at worlds 1 .. 64 and explicit cuts: a single
candidate alone, a cut directly behind the first copy of the cheapest tie group, directly before the winner, empty ranks in the middle and
last); what they cover is asserted on the oracle in tests/test_shard_combine_host.py.

test_exchange_*: the combine step on THE COSTS THE DEVICE RETURNED -- winner and best_cost bits against tests/_ladder.py:
reference_selection over the concatenation of the shards' fetch_status(), owner = the rank whose range holds the winner, counters the
sums, rows and coefficients the owner's, the summed second message that selection's count.

test_costs_do_not_depend_on_the_cut: every shard's cost[] equals the slice of the unsharded plan's as uint64 (status words equal up to
the relaxation of the cost-ordered stage: tests/_lazy.py), at default options, and the combined result is the unsharded plan's.  This is
what option "shard_policy" = 1 (the default) is for: lanes per candidate and single launch / two kernels -- the two choices that decide
the bits of a cost -- follow the grid, not the range.  test_range_policy_tells_producers_apart is the control: under
"shard_policy" = 0 the same partitions meet at least two producers (read back: options "last_lanes", "last_single_launch") and at
least one candidate's cost bits differ from the whole plan's, i.e. the scenes can tell the producers apart.  Two scenes cannot and are
left out of the control, not of the test: all_collide_44 (every range of 44 candidates is below every threshold) and none_feasible
(no candidate has a cost)."""
import types

import numpy as np
import pytest

import _ladder as LD
import _shards as SH
from _lazy import lazy_relaxed
from commonroad_rp_amd import _capi
from commonroad_rp_amd.distributed import _DeviceBlock, local_collisions_before

pytestmark = pytest.mark.gpu

EXCHANGE_SCENES = SH.SMALL_SCENES + (LD.N40,)
G48 = ("g48_rank6528", "g48_rank24080")         # 47 520 candidates: the whole plan keeps no rows and takes the cost-ordered stage, its shards do not
G48_WORLDS = (2, 3, 16)
CUT_SCENES = SH.SMALL_SCENES + G48 + (LD.N40,)
CONTROL_SCENES = tuple(n for n in CUT_SCENES if n not in ("all_collide_44", "none_feasible"))
PATH_EAGER = 0


@pytest.fixture(scope="module")
def ctx():
    _capi.set_default_options(None)
    c = _capi.RpContext(0)
    yield c
    assert c.get_option("wait_fallbacks") == 0
    c.close()
    _capi.set_default_options(None)


@pytest.fixture(autouse=True)
def _reset(ctx):
    yield
    _capi.set_default_options(None)
    ctx.set_collision_path(_capi.COLLISION_AUTO)


def _bits(x):
    return int(np.float64(x).view(np.uint64))


def _cut_partitions(name):
    if name in G48:
        C = LD.SCENES[name].n_candidates
        return [(f"world{w}", SH.by_world(C, w)) for w in G48_WORLDS]
    return SH.partitions(name, SH.CUT_WORLDS)


def _producer(ctx):
    return ctx.get_option("last_lanes"), ctx.get_option("last_single_launch")


def _plan_whole(ctx, name):
    sc, run = LD.oracle_run(name)
    sc.setup(ctx)
    out = ctx.plan(sc.inputs)
    status, cost = ctx.fetch_status()
    fixed, _ = lazy_relaxed(status, cost, run, ctx, out)
    return types.SimpleNamespace(out=out, status=status, cost=cost, fixed=fixed, producer=_producer(ctx), path=ctx.last_path())


def _plan_shards(ctx, name, ranges, gather=False):
    """every range planned in turn on the one context: outputs, status / cost arrays, producers, paths; gather: the device result
    block of rank r copied into row r of one message tensor"""
    import torch
    sc, run = LD.oracle_run(name)
    sc.setup(ctx)
    dev = torch.device("cuda", 0)
    x = types.SimpleNamespace(outs=[], status=[], cost=[], fixed=[], producers=[], paths=[], msgs=None)
    for r, (lo, hi) in enumerate(ranges):
        out = ctx.plan(sc.inputs, lo, hi)
        if gather:
            ptr, nbytes, rows_ok = ctx.result_device()
            assert rows_ok and ptr and nbytes == (45 + 14 * (sc.inputs.params.N + 1)) * 8
            if x.msgs is None:
                x.msgs = torch.zeros((len(ranges), nbytes // 8), dtype=torch.float64, device=dev)
            x.msgs[r].copy_(torch.as_tensor(_DeviceBlock(ptr, nbytes), device=dev))
            torch.cuda.synchronize()          # (the block is the context's: the next plan overwrites it)
        status, cost = ctx.fetch_status()
        fixed, _ = lazy_relaxed(status, cost, types.SimpleNamespace(status=run.status[lo:hi]), ctx, out, lo)
        x.outs.append(out); x.status.append(status); x.cost.append(cost); x.fixed.append(fixed)
        x.producers.append(_producer(ctx)); x.paths.append(ctx.last_path())
    return x


def _exchange(ctx, name, ranges):
    """both messages of one sharded step: the shards' data, the combined result seen from the last rank and from rank 0, the owners,
    the summed second message"""
    import torch
    sc, _ = LD.oracle_run(name)
    world = len(ranges)
    x = _plan_shards(ctx, name, ranges, gather=True)
    stream = torch.cuda.current_stream().cuda_stream
    x.glob_last, x.owner_last, x.rows_last = ctx.combine_results(x.msgs.data_ptr(), world, stream)
    x.total_before = 0
    for r, (lo, hi) in enumerate(ranges):
        out = ctx.plan(sc.inputs, lo, hi)
        if r == 0:
            x.glob0, x.owner0, x.rows0 = ctx.combine_results(x.msgs.data_ptr(), world, stream)
        x.total_before += local_collisions_before(ctx, out, x.glob0, r == x.owner0)
    return x


def _check_exchange(x, ranges, what, replicated=False):
    """the combine step against the plain selection over what the shards returned"""
    cost = np.concatenate(x.cost)
    status = np.concatenate(x.status)
    lab = status & 3
    if replicated:      # every non-empty rank holds the whole grid: the selection is the first rank's, the counters are the sums
        wi, wc, nb = LD.reference_selection(x.cost[0], x.status[0] & 3)
        want_owner = 0 if wi >= 0 else -1
    else:
        wi, wc, nb = LD.reference_selection(cost, lab)
        want_owner = SH.rank_of(ranges, wi)
    for glob, owner, rows_ok in ((x.glob_last, x.owner_last, x.rows_last), (x.glob0, x.owner0, x.rows0)):
        assert glob.best_index == wi, (what, glob.best_index, wi)
        assert owner == want_owner, (what, owner, want_owner)
        assert rows_ok, what
        if wi >= 0:
            assert _bits(glob.best_cost) == _bits(wc), what
            o = x.outs[owner]
            assert o.best_index == wi and _bits(o.best_cost) == _bits(wc), what
            np.testing.assert_array_equal(glob.best_states, o.best_states, err_msg=str(what))
            np.testing.assert_array_equal(glob.best_lon_coeffs, o.best_lon_coeffs, err_msg=str(what))
            np.testing.assert_array_equal(glob.best_lat_coeffs, o.best_lat_coeffs, err_msg=str(what))
            assert glob.best_lat_T == o.best_lat_T, what
        else:
            assert owner == -1 and np.isnan(glob.best_cost) and glob.best_states is None, what
        assert glob.n_candidates == sum(o.n_candidates for o in x.outs) == len(cost), what
        assert glob.n_feasible == sum(o.n_feasible for o in x.outs) == np.count_nonzero((lab == 1) | (lab == 3)), what
        np.testing.assert_array_equal(glob.reason_counts, sum(o.reason_counts for o in x.outs), err_msg=str(what))
        np.testing.assert_array_equal(glob.reason_counts, LD.reason_counts(status), err_msg=str(what))
        if all(p == PATH_EAGER for p in x.paths):      # (a cost-ordered plan labels, and counts, only what it had to look at)
            assert glob.n_collision == sum(o.n_collision for o in x.outs) == np.count_nonzero(lab == 3), what
    if not replicated:
        assert x.total_before == nb, (what, x.total_before, nb)
    return wi, wc, nb


def _check_against_oracle(x, name, ranges, what):
    """the device's shards against the oracle's: labels exact on eager plans, the same candidates have a cost, costs within the
    project's contract -- so that what tests/test_shard_combine_host.py asserts of the partitions holds of the device's data"""
    _, run = LD.oracle_run(name)
    for (lo, hi), status, cost, path in zip(ranges, x.status, x.cost, x.paths):
        oc = run.cost[lo:hi]
        have = ~np.isnan(oc)
        assert np.array_equal(np.isnan(cost), ~have), what
        assert np.all(np.abs(cost[have] - oc[have]) <= 1e-9 * np.abs(oc[have])), what
        if path == PATH_EAGER:
            np.testing.assert_array_equal(status & 0x7F, run.status[lo:hi] & 0x7F, err_msg=str(what))


# ---- B: the combine step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXCHANGE_SCENES)
def test_exchange_on_ties_and_empty_ranks(ctx, name):
    C = LD.oracle_run(name)[0].n_candidates
    seen = set()
    for tag, ranges in SH.partitions(name, SH.DEVICE_WORLDS):
        SH.check_partition(ranges, C)
        what = (name, tag)
        x = _exchange(ctx, name, ranges)
        _check_against_oracle(x, name, ranges, what)
        _check_exchange(x, ranges, what)
        seen |= SH.facts(np.concatenate(x.cost), np.concatenate(x.status) & 3, ranges)
    assert {"empty_middle", "empty_last"} <= seen
    for tag, ranges in SH.replicated(name):
        x = _exchange(ctx, name, ranges)
        _check_exchange(x, ranges, (name, tag), replicated=True)
    assert ctx.get_option("wait_fallbacks") == 0


@pytest.mark.parametrize("name", ["mirror_rank721", "all_collide_4248"])
def test_exchange_under_the_eager_collision_path(ctx, name):
    """RP_COLLISION_EAGER: every participant reports RP_PATH_EAGER, so n_collision of the combined result is asserted as the sum"""
    ctx.set_collision_path(_capi.COLLISION_EAGER)
    for tag, ranges in SH.partitions(name, (3, 64)):
        x = _exchange(ctx, name, ranges)
        assert all(p == PATH_EAGER for p in x.paths), (name, tag, x.paths)
        _check_exchange(x, ranges, (name, tag))
        assert x.glob0.n_collision == LD.oracle_run(name)[1].out.n_collision


def test_world_beyond_the_limit_is_refused_and_the_context_stays_usable(ctx):
    import torch
    name = "rank72"
    sc, _ = LD.oracle_run(name)
    sc.setup(ctx)
    out = ctx.plan(sc.inputs)
    ptr, nbytes, _ = ctx.result_device()
    msgs = torch.zeros((65, nbytes // 8), dtype=torch.float64, device=torch.device("cuda", 0))
    msgs[:] = torch.as_tensor(_DeviceBlock(ptr, nbytes), device=msgs.device)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    for world in (65, 0, -1):
        with pytest.raises(_capi.RpError, match=r"rp_combine_results -> -1: .*world size out of range"):
            ctx.combine_results(msgs.data_ptr(), world, stream)
    glob, owner, rows_ok = ctx.combine_results(msgs.data_ptr(), 64, stream)      # (64 equal messages: the first rank owns the winner)
    assert (glob.best_index, owner, rows_ok) == (out.best_index, 0, True) and _bits(glob.best_cost) == _bits(out.best_cost)
    assert glob.n_candidates == 64 * out.n_candidates
    np.testing.assert_array_equal(glob.best_states, out.best_states)
    again = ctx.plan(sc.inputs)
    assert again.best_index == out.best_index and _bits(again.best_cost) == _bits(out.best_cost)
    assert ctx.get_option("wait_fallbacks") == 0


# ---- C: independence of the cut -----------------------------------------------------------------------------------------------------------
def compare_with_whole(ctx, name, whole, tag, ranges):
    """figures of one partition against the unsharded plan (asserted by the test; profiles/probe_shard_policy.py prints them)"""
    x = _exchange(ctx, name, ranges)
    cost = np.concatenate(x.cost)
    fixed = np.concatenate(x.fixed)
    g = x.glob0
    return types.SimpleNamespace(
        x=x, tag=tag,
        cost_bits_differ=int(np.count_nonzero(cost.view(np.uint64) != whole.cost.view(np.uint64))),
        status_differ=int(np.count_nonzero((fixed & 0x7F) != (whole.fixed & 0x7F))),
        producers=sorted(set(x.producers[r] for r, (lo, hi) in enumerate(ranges) if hi > lo)),
        winner=(g.best_index, whole.out.best_index),
        winner_cost_bits_equal=(np.isnan(g.best_cost) and np.isnan(whole.out.best_cost)) or _bits(g.best_cost) == _bits(whole.out.best_cost),
        before=(x.total_before, whole.out.n_collision_before_best),
        feasible=(g.n_feasible, whole.out.n_feasible))


@pytest.mark.parametrize("name", CUT_SCENES)
def test_costs_do_not_depend_on_the_cut(ctx, name):
    whole = _plan_whole(ctx, name)
    for tag, ranges in _cut_partitions(name):
        what = (name, tag)
        f = compare_with_whole(ctx, name, whole, tag, ranges)
        print(what, "cost bits differ:", f.cost_bits_differ, "status differ:", f.status_differ, "producers:", f.producers, "whole:", whole.producer,
              "winner:", f.winner, "before:", f.before)
        # the slice comparison: fails whenever two producers met, not only when a winner happened to flip
        assert f.cost_bits_differ == 0, (what, f.cost_bits_differ, f.producers, whole.producer)
        assert f.status_differ == 0, (what, f.status_differ)
        assert f.producers == [whole.producer], (what, f.producers, whole.producer)
        x, g = f.x, f.x.glob0
        _check_exchange(x, ranges, what)
        assert g.best_index == x.glob_last.best_index == whole.out.best_index, what
        assert f.winner_cost_bits_equal, what
        assert g.n_candidates == whole.out.n_candidates and g.n_feasible == whole.out.n_feasible, what
        np.testing.assert_array_equal(g.reason_counts, whole.out.reason_counts, err_msg=str(what))
        assert x.total_before == whole.out.n_collision_before_best, what
        if whole.out.best_index >= 0:
            np.testing.assert_array_equal(g.best_states, whole.out.best_states, err_msg=str(what))
            np.testing.assert_array_equal(g.best_lon_coeffs, whole.out.best_lon_coeffs, err_msg=str(what))
            np.testing.assert_array_equal(g.best_lat_coeffs, whole.out.best_lat_coeffs, err_msg=str(what))
    assert ctx.get_option("shard_policy") == 1 and ctx.get_option("wait_fallbacks") == 0


@pytest.mark.parametrize("name", CONTROL_SCENES)
def test_range_policy_tells_producers_apart(ctx, name):
    whole1 = _plan_whole(ctx, name)                       # by grid (default)
    _capi.set_default_options({"shard_policy": 0})        # by range
    assert ctx.get_option("shard_policy") == 0
    whole0 = _plan_whole(ctx, name)
    # a whole-grid plan chooses the same either way
    assert whole0.producer == whole1.producer and np.array_equal(whole0.cost.view(np.uint64), whole1.cost.view(np.uint64)), name
    assert whole0.producer[0] in (16, 32, 64) and whole0.producer[1] in (0, 1)
    producers, differ = {whole0.producer}, 0
    for tag, ranges in _cut_partitions(name):
        x = _plan_shards(ctx, name, ranges)
        producers |= set(x.producers[r] for r, (lo, hi) in enumerate(ranges) if hi > lo)
        differ += int(np.count_nonzero(np.concatenate(x.cost).view(np.uint64) != whole0.cost.view(np.uint64)))
    print(name, "producers under shard_policy 0:", sorted(producers), "cost bits that differ from the whole plan's:", differ)
    assert len(producers) >= 2, (name, producers)
    assert differ >= 1, name
