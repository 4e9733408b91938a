"""rp_eval_kernel (16 lanes per candidate), rp_cost_kernel (one lane per candidate) and rp_chunk_kernel (one lane per candidate and
step block of 16) agree BIT FOR BIT: the same status words, the same cost bits, the same winner and counters (DESIGN.md section 2,
"Bit-identity between kernels"; the comment above cost_terms in csrc/rp_kernels.h).  Which of them evaluates a batch is decided by
its size, horizon and collision level, and the cost-ordered collision stage takes costs from one and labels from another, so a
one-ulp disagreement is a different winner on a near-tie -- and passes every comparison with the oracle (1e-8 relative).

Everything goes through the C ABI; no oracle runs here (tests/_bitid.py: selections, comparison, cases).  Every plan asserts
rp_last_kernel(): a module that compares rp_eval_kernel with itself does not pass.  No tolerance on the three kernels anywhere; the
launch variants outside the contract (32 / 64 lanes per candidate, single launch) are held to the summation bound 2 (n - 1) 2^-53.

Mutation check (done once on a scratch copy, not committed): with the first level of sum16_group_order's tree pairing neighbouring partial
sums instead of those eight apart, the edge matrix, the random cases and the workloads of this module fail on cost bits (27 of 28 cases)
while tests/test_fuzz_parity.py passes on the same build."""
import types

import numpy as np
import pytest

import _bitid as B
from commonroad_rp_amd._capi import FLAG_SKIP_COLLISION

RANDOM_SEEDS = range(1000, 1300)   # (tests/test_fuzz_parity.py takes 0 .. 699)


# ---- without a GPU: the comparison itself, and that the cases are what they claim to be -----------------------------------------
def _out(**kw):
    base = dict(best_index=3, best_cost=2.5, n_feasible=4, n_collision=1, n_collision_before_best=0, reason_counts=np.arange(8))
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_comparison_reports_what_it_must():
    nan = float("nan")
    st = np.array([1, 3, 2 | (3 << 4) | (31 << 8), 0 | (6 << 4) | (16 << 8)], dtype=np.uint32)
    cs = np.array([1.25, 7.0, nan, nan])
    assert B.status_cost_differences(st, cs, st.copy(), cs.copy()) == []                      # equal NaNs are equal
    other_nan = cs.copy()
    other_nan.view(np.uint64)[2] ^= np.uint64(1)                                              # ... whatever their payload
    assert np.isnan(other_nan[2]) and B.status_cost_differences(st, cs, st, other_nan) == []
    flipped = cs.copy()
    flipped.view(np.uint64)[0] ^= np.uint64(1)                                                # one ulp: 1e-16 relative
    found = B.status_cost_differences(st, cs, st, flipped)
    assert len(found) == 1 and "finite costs differ in their bits" in found[0] and "first at 0" in found[0]
    step = st.copy()
    step[2] = 2 | (3 << 4) | (32 << 8)                                                        # the same failure one step later
    found = B.status_cost_differences(st, cs, step, cs)
    assert len(found) == 1 and "status words differ" in found[0] and "step 31" in found[0] and "step 32" in found[0]
    one_sided = cs.copy()
    one_sided[3] = 4.0
    found = B.status_cost_differences(st, cs, st, one_sided)
    assert len(found) == 1 and "NaN on one side only" in found[0] and "first at 3" in found[0]
    assert B.status_cost_differences(st, cs, st[:3], cs[:3])                                  # different lengths
    # the plan's result: winner, cost bits, counters
    assert B.output_differences(_out(), _out()) == []
    assert B.output_differences(_out(best_index=-1, best_cost=nan), _out(best_index=-1, best_cost=nan)) == []
    assert len(B.output_differences(_out(), _out(best_cost=float(np.nextafter(2.5, 3.0))))) == 1
    assert len(B.output_differences(_out(), _out(best_cost=nan))) == 1
    assert len(B.output_differences(_out(), _out(best_index=4))) == 1
    assert len(B.output_differences(_out(), _out(n_collision_before_best=1))) == 1
    assert len(B.output_differences(_out(), _out(reason_counts=np.arange(8)[::-1]))) == 1
    assert B.output_differences(_out(), _out(n_collision=2), B.OUT_FIELDS_COST_ORDERED) == []
    # the bound of the variants outside the contract: status exact, costs within 2 (n - 1) 2^-53
    a = B.Run(st, cs, _out())
    assert B.bound_differences(a, B.Run(st, flipped, _out()), N=30)[0] == []
    assert B.bound_differences(a, B.Run(st, cs * (1.0 + 1e-13), _out()), N=30)[0]
    assert B.bound_differences(a, B.Run(step, cs, _out()), N=30)[0]
    assert B.bound_differences(a, B.Run(st, one_sided, _out()), N=30)[0]
    assert B.summation_bound(60) == 120 * 2.0 ** -53


def test_edge_matrix_covers_every_axis():
    """Every value of every axis of the edge matrix appears in both velocity modes at horizons all three kernels serve."""
    specs = B.edge_matrix()
    assert all(B.chunk_applies(s.n_steps - 1) for s in specs) and not any(B.chunk_applies(n - 1) for n in B.OTHER_HORIZONS)
    assert B.selections_for(60) == ["eval16", "eval16_wave_wg", "lane", "chunk"] and B.selections_for(112) == ["eval16", "eval16_wave_wg", "lane"]
    for low in (False, True):
        mine = [s for s in specs if s.low == low]
        assert {s.n_steps for s in mine} == set(B.CHUNK_HORIZONS)
        for axis, values in (("start", B.STARTS), ("obstacles", B.OBSTACLES), ("mask", B.MASKS), ("factor", B.FACTORS), ("cost", B.COSTS)):
            assert {getattr(s, axis) for s in mine} == set(values), (low, axis)
        assert {s.n_steps for s in B.edge_matrix(B.OTHER_HORIZONS) if s.low == low} == set(B.OTHER_HORIZONS)
    assert len({s.id for s in specs}) == len(specs)


@pytest.mark.parametrize("n_steps", [2, 3, 16, 17, 33, 49, 112, 130])
def test_edge_case_extends_at_every_block_boundary(n_steps):
    """One batch holds the first extended steps 16 k - 1, 16 k, 16 k + 1, 16 k + 2 of every step block k, and N + 1; a wavefront of 64
    consecutive candidates covers more than one of them."""
    want = B.traj_len_grid(n_steps)
    blocks = (n_steps + 15) // 16
    for k in range(1, blocks + 1):
        for t in (16 * k - 1, 16 * k, 16 * k + 1, 16 * k + 2):
            assert (t in want) == (3 <= t <= n_steps)
    assert n_steps in want
    inp, _, _ = B.edge_case(B.EdgeSpec(n_steps, False, "lateral", "none", 31, 1, "speed"))
    assert list(inp.traj_len) == want and inp.params.N + 1 == n_steps
    assert len(inp.L) * len(inp.D) < 64 and (len(inp.L) * len(inp.D)) % 64 != 0


def test_random_seed_range_reaches_the_chunk_kernel():
    from _fuzz import random_case
    horizons = [random_case(seed)[3]["N"] for seed in RANDOM_SEEDS]
    assert len(horizons) == 300 and sum(B.chunk_applies(N) for N in horizons) >= 200
    assert min(RANDOM_SEEDS) >= 700


# ---- on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = B.new_context(0)
    yield c
    c.close()


def _compare_all(ctx, inp, co, obs, what, lo=0, hi=-1, want_chunk=None):
    ctx.set_coordinate_system(co)
    ctx.set_obstacles(obs)
    eager, compared = B.compare_kernels(ctx, inp, lo, hi, what)
    if want_chunk is not None:
        assert ("chunk" in compared) == want_chunk, (what, compared)
    assert "lane" in compared and "eval16_wave_wg" in compared
    if not obs.empty and not (inp.params.flags & FLAG_SKIP_COLLISION):
        B.compare_cost_ordered(ctx, inp, eager, lo, hi, what)
    return eager


@pytest.mark.gpu
@pytest.mark.parametrize("spec", B.edge_matrix(), ids=lambda s: s.id)
def test_edge_matrix_three_kernels(ctx, spec):
    """Horizons of 2 .. 7 step blocks around the block boundaries; start states, collision levels, constraint masks, factors and cost
    functions rotating (tests/_bitid.py: edge_matrix).  eval16, its one-wavefront launch, lane and chunk; then the cost-ordered stage."""
    inp, co, obs = B.edge_case(spec)
    _compare_all(ctx, inp, co, obs, spec.id, want_chunk=True)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", B.edge_matrix(B.OTHER_HORIZONS), ids=lambda s: s.id)
def test_edge_matrix_eval_against_lane(ctx, spec):
    """Horizons rp_chunk_kernel does not serve (one step block; more than seven): eval16, its one-wavefront launch and lane."""
    inp, co, obs = B.edge_case(spec)
    _compare_all(ctx, inp, co, obs, spec.id, want_chunk=False)


@pytest.mark.gpu
@pytest.mark.parametrize("low", [False, True], ids=["hv", "lv"])
def test_first_failure_on_block_edges(ctx, low):
    """First failing step and first out-of-domain step on the last step of a block and on the first step of the next one -- checked on
    what eval16 returns, so that a batch that stops containing them fails instead of passing empty."""
    inp, co, obs = B.failure_case(low)
    for extra in (0, FLAG_SKIP_COLLISION):
        eager = _compare_all(ctx, B.production(inp, extra), co, obs, f"failures {'lv' if low else 'hv'} flags {extra}", want_chunk=True)
        kin, ood = B.block_edge_steps(eager.status)
        assert {15, 0} <= kin, f"first failing steps (mod 16) of the batch: {sorted(kin)}"
        assert {15, 0} <= ood, f"first out-of-domain steps (mod 16) of the batch: {sorted(ood)}"
        assert (~np.isnan(eager.cost)).sum() >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("low", [False, True], ids=["hv", "lv"])
def test_batch_shapes_and_sharded_ranges(ctx, low):
    """1, 63, 64, 65 candidates, a batch beyond 4 096 that is no multiple of 64, and ranges whose ends are off the multiples of 64 and
    of nD: the wavefronts of the lane kernels straddle (T, longitudinal sample) pairs and end inside one."""
    spec = B.EdgeSpec(49, low, "lateral", "dynamic", 31, 1, "speed")
    inp, co, obs = B.edge_case(spec, nL=37, nD=11)
    C, nD = inp.n_candidates, len(inp.D)
    assert C > 4096 and C % 64 != 0
    ranges = [(0, 1), (7, 70), (100, 164), (811, 876), (0, C), (333, 2990), (2990, C), (C - 1, C)]
    assert [hi - lo for lo, hi in ranges[:4]] == [1, 63, 64, 65]
    assert all(lo % 64 and lo % nD and hi % 64 and hi % nD for lo, hi in ranges[5:6])
    for lo, hi in ranges:
        eager = _compare_all(ctx, inp, co, obs, f"{spec.id} range [{lo}, {hi})", lo, hi, want_chunk=True)
        assert len(eager.status) == hi - lo


@pytest.mark.gpu
def test_random_cases_three_kernels(ctx):
    """tests/_fuzz.py's generator on 300 seeds the oracle fuzz does not take, as production-mode plans without the collision query and
    with the eager one.  What was compared is counted: the caps below fail a run that compared less."""
    chunk = winners = finite = 0
    for seed in RANDOM_SEEDS:
        c, w, f = B.compare_random_case(ctx, seed)
        chunk += c
        winners += w
        finite += f
    counts = f"rp_chunk_kernel ran on {chunk} of {len(RANDOM_SEEDS)} seeds, {winners} seeds had a winner, {finite} finite costs compared"
    print(counts)
    assert chunk >= 200 and winners >= 30 and finite >= 10000, counts


# The single-launch variant is held to 1e-12 relative (the figure tests/test_options_abi.py uses for best_cost across launch paths)
# instead of the summation bound: its per-step terms are NOT eval16's numbers.  It computes the longitudinal profile rows in its own
# prologue (lon_step_part) where the two-kernel path takes rp_lon_kernel's (lon_step); at horizons of one step block the values of
# the longitudinal polynomial (s, s_dot, s_ddot) come out with other last bits there, the lateral ones and everything at longer
# horizons are bit-equal.  Measured on these seeds: up to 1.33 x the summation bound (seed 1221; 3.2e-15 relative at n = 13 on seed 1084).
# DESIGN.md section 2 records it.
VARIANT_BOUND = {"g32": None, "g64": None, "single_launch": 1e-12}   # None: summation_bound(N)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(B.BOUND_VARIANTS))
def test_other_launch_variants_within_summation_bound(ctx, variant):
    """32 / 64 lanes per candidate add the per-step terms of eval16 in another order: status words equal, costs within
    2 (n - 1) 2^-53 relative, n = N + 1 steps (tests/_bitid.py: summation_bound).  The single-launch variant: see VARIANT_BOUND.
    Not part of the bit-identity contract."""
    worst = (0.0, None)
    finite = 0
    for seed in RANDOM_SEEDS:
        inp, co, obs, info = B.random_production_case(seed)
        ctx.set_coordinate_system(co)
        ctx.set_obstacles(obs)
        for extra in (FLAG_SKIP_COLLISION, 0):
            i2 = B.production(inp, extra)
            ref = B.run_selection(ctx, i2, "eval16")
            run = B.run_variant(ctx, i2, variant)
            found, dev = B.bound_differences(ref, run, info["N"], VARIANT_BOUND[variant])
            worst = max(worst, (dev / B.summation_bound(info["N"]), seed))
            finite += int((~np.isnan(ref.cost)).sum())
            assert not found, f"{variant} / eval16, seed {seed} flags {extra} {info}: " + "; ".join(found)
    print(f"{variant}: {finite} finite costs, largest deviation {worst[0]:.3f} of the summation bound (seed {worst[1]})")
    assert finite >= 5000


def _workload(name):
    from commonroad_rp_amd import workloads as W
    return W.WORKLOADS[name[:-2]](road_boundary=True) if name.endswith("rb") else W.WORKLOADS[name]()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg3f", "cfg3rb", "cfg4"])
def test_workload_scale(ctx, name):
    """The benchmark workloads at full size, without the collision query and with the eager one, by every kernel (cfg4: 512 064
    candidates in seven step blocks); cfg3 and cfg3f also through the cost-ordered stage and the bounded sweep."""
    w = _workload(name)
    w.setup(ctx)
    inp = B.production(w.inputs)
    for extra in (FLAG_SKIP_COLLISION, 0):
        i2 = B.production(inp, extra)
        eager, compared = B.compare_kernels(ctx, i2, what=f"{name} flags {extra}")
        assert set(compared) == {"eval16_wave_wg", "lane", "chunk"} and compared["chunk"] > 0, (name, compared)
        if extra == 0 and name in ("cfg3", "cfg3f"):
            B.compare_cost_ordered(ctx, i2, eager, what=name)
