"""The fixed-stride variant of the 16-lane rp_eval_kernel that stores state rows (csrc/rp_kernels.h: ROW64 -- rows of 64 doubles,
no split tail; row stores from one address, cost parameters in one fetch, cost terms and the static-grid cell once per step block)
against the generic variant, pinned with the option "fixed_stride" = 0: status words, cost bits and every element of every state
row are the SAME BITS -- the variant changes how the step block is issued, not what it computes.  Then both against the CPU oracle
at the tolerances of tests/test_gpu_parity.py.

Everything goes through the C ABI on the two-kernel path with 16 lanes per candidate (tests/_paths.py: "two_kernel").  Which variant
evaluated a batch is read back (read-only option "last_fixed_stride") and asserted: a module that compares the generic variant with
itself does not pass.

Shapes.  N + 1 = 61 and 64 have rows of 64 doubles under the default layout (last step block partial / full).  N + 1 = 17 and 49 end
one step into a block and get the split tail by default (rows of 16 / 48 doubles): they take the fixed-stride variant only with the
layout option "tail_split" = 0, where 49 steps are padded to 64 -- 17 steps are padded to 32 and stay generic either way.  N + 1 = 33
and 101 never have rows of 64 doubles and must take the generic path under both layouts, and still pass.  Every horizon runs under
both layouts.  Batches are ranges of 37 candidates (a wavefront of four candidates and a workgroup of sixteen partly filled) and of
4 099 (more than one workgroup per (T, longitudinal sample) pair: 37 lateral samples per pair), starting off the multiples of 16.

The time samples of a batch (tests/_bitid.py: traj_len_grid) put the last valid step L - 1 on the last lane of a step block, on the
first lane of the next and one and two lanes in (L = 16 k - 1, 16 k, 16 k + 1, 16 k + 2 for every block k) and hold L = N + 1 (no
extension): L - 1 in the middle of a block, L a multiple of 16, L = N + 1."""
import functools

import numpy as np
import pytest

import _bitid as B
from _paths import options
from commonroad_rp_amd._capi import (PlanInputs, RpContext, copy_params, make_cost, COST_DEFAULT, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL)

STATE_ATOL = 1e-6    # tests/test_gpu_parity.py
COST_RTOL = 1e-9

HORIZONS = (17, 49, 61, 64, 33, 101)                 # N + 1
LAYOUTS = {"default": {}, "unsplit": {"tail_split": 0}}
FIXED = {(61, "default"), (64, "default"), (49, "unsplit"), (61, "unsplit"), (64, "unsplit")}   # where the rows lie 64 doubles apart
SIZES = (37, 4099)
FIRST = 5                                            # first candidate of a range: off the multiples of 4, 16 and 37
N_LATERAL = 37
COLLISION = ("none", "dynamic", "static")            # collision levels 0, 1, 2 (tests/_bitid.py: edge_obstacles)
COSTS = {"plain": (False, False), "speed": (True, False), "s": (False, True), "speed_and_s": (True, True)}   # has_speed, has_s
MODES = {"draw": FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL, "materialise": FLAG_MATERIALIZE_ALL}
BLOCKS = (256, 64)                                   # threads per workgroup of the evaluation kernel
TWO_KERNEL_16 = {"fused_lon": 0, "lanes": 16}


def row_stride(n_steps, layout):
    """doubles between the state rows of the two-kernel path with 16 lanes per candidate (csrc/rp_host.hip: state_layout)"""
    r = n_steps % 16
    if layout == "default" and 0 < r <= 8 and n_steps - r >= 16:
        return n_steps - r   # split tail
    return (n_steps + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def scene(n_steps, collision, low):
    """inputs (without cost function and flags), coordinate system and obstacle tables: at least FIRST + 4 099 candidates"""
    n_t = len(B.traj_len_grid(n_steps))
    n_l = -(-(FIRST + max(SIZES)) // (n_t * N_LATERAL))
    spec = B.EdgeSpec(n_steps, low, "lateral", collision, 31, 1, "plain")
    inp, co, obs = B.edge_case(spec, nL=n_l, nD=N_LATERAL)
    assert inp.n_candidates >= FIRST + max(SIZES) and len(inp.D) == N_LATERAL
    return inp, co, obs


def with_cost_and_flags(inp, cost_name, flags):
    has_speed, has_s = COSTS[cost_name]
    p = copy_params(inp.params)
    p.flags = flags
    cost = make_cost(COST_DEFAULT, w_a=5.0, desired_speed=float(p.x0_lon[1]) + 1.0 if has_speed else None, desired_d=0.5,
                     desired_s=float(p.x0_lon[0]) + 20.0 if has_s else None)
    return PlanInputs(p, cost, inp.T, inp.traj_len, inp.L, inp.D)


def combos(n_steps):
    """(collision level, cost, mode, size, block, low-velocity mode): collision levels x cost functions x modes x sizes in full, the
    workgroup size and the velocity mode rotating against them -- 48 plans per horizon and layout"""
    out = []
    for ci, collision in enumerate(COLLISION):
        for k, cost in enumerate(COSTS):
            for mi, mode in enumerate(MODES):
                for si, size in enumerate(SIZES):
                    out.append((collision, cost, mode, size, BLOCKS[(ci + k + mi + si + n_steps) % 2], bool((k + (ci + si) // 2 + mi) % 2)))
    return out


def candidate_range(inp, size):
    """`size` candidates from the middle of the batch on (the first time samples are short trajectories, most of them infeasible),
    starting FIRST behind a multiple of 16"""
    lo = (inp.n_candidates // 2 if size < 100 else 0) // 16 * 16 + FIRST
    assert lo + size <= inp.n_candidates
    return lo, lo + size


def test_cases_are_what_they_claim():
    """without a GPU: the layouts the cases rely on, and that the combinations cover every axis at every collision level"""
    assert {(n, l) for n in HORIZONS for l in LAYOUTS if row_stride(n, l) == 64 and n > 16} == FIXED
    assert row_stride(17, "default") == 16 and row_stride(17, "unsplit") == 32 and row_stride(49, "default") == 48
    assert row_stride(33, "default") == 32 and row_stride(33, "unsplit") == 48 and row_stride(101, "default") == 96 and row_stride(101, "unsplit") == 112
    for n in HORIZONS:
        cs = combos(n)
        assert len(set(cs)) == len(cs) == 48
        for axis, values in ((0, COLLISION), (1, COSTS), (2, MODES)):
            for v in values:   # every collision level, cost function and mode meets both sizes, workgroup sizes and velocity modes
                mine = [c for c in cs if c[axis] == v]
                assert {c[3] for c in mine} == set(SIZES) and {c[4] for c in mine} == set(BLOCKS) and {c[5] for c in mine} == {False, True}
        tl = B.traj_len_grid(n)   # L = N + 1, L a multiple of 16, L - 1 inside a block
        assert n in tl and any(t % 16 == 0 for t in tl) and any((t - 1) % 16 not in (0, 15) for t in tl if t < n)
    inp, _, _ = scene(61, "none", False)
    assert inp.params.N == 60 and inp.n_candidates >= FIRST + 4099
    assert list(inp.traj_len) == B.traj_len_grid(61)


@pytest.fixture(scope="module")
def ctx():
    with options(**TWO_KERNEL_16):
        c = RpContext(0)
        yield c
        c.close()


def run(ctx, inp, lo, hi, block, fixed_stride):
    ctx.set_option("eval_block", block)
    ctx.set_option("fixed_stride", fixed_stride)
    out = ctx.plan(inp, lo, hi)
    assert ctx.last_kernel() == "rp_eval_kernel" and ctx.last_path() == 0
    status, cost = ctx.fetch_status()
    return out, status, cost, ctx.fetch_states(), ctx.get_option("last_fixed_stride")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n_steps", HORIZONS)
def test_fixed_stride_variant_is_the_generic_one_bit_for_bit(ctx, n_steps, layout):
    from oracle import oracle
    for k, v in dict({"tail_split": 1}, **LAYOUTS[layout]).items():
        ctx.set_option(k, v)
    defined_rows = finite = collided = extended = 0
    for collision, cost_name, mode, size, block, low in combos(n_steps):
        what = f"N + 1 = {n_steps}, {layout} layout, {collision}, cost {cost_name}, {mode}, block {block}, {'low' if low else 'high'} velocity, {size} candidates"
        base, co, obs = scene(n_steps, collision, low)
        inp = with_cost_and_flags(base, cost_name, MODES[mode])
        ctx.set_coordinate_system(co)
        ctx.set_obstacles(obs)
        lo, hi = candidate_range(inp, size)
        gen = run(ctx, inp, lo, hi, block, 0)
        fix = run(ctx, inp, lo, hi, block, 1)
        assert gen[4] == 0, what
        assert fix[4] == int((n_steps, layout) in FIXED), what   # the variant under test ran exactly where the rows lie 64 doubles apart
        assert len(fix[1]) == size and fix[3].shape == (size, 14, n_steps), what
        # -- bit for bit: status, cost, every state row; the plan's result
        found = B.status_cost_differences(gen[1], gen[2], fix[1], fix[2]) + B.output_differences(gen[0], fix[0])
        assert not found, what + ": " + "; ".join(found)
        assert same_bits(gen[3], fix[3]), what + f": {int((gen[3].view(np.uint64) != fix[3].view(np.uint64)).sum())} state elements differ"
        if gen[0].best_index >= 0:
            assert same_bits(gen[0].best_states, fix[0].best_states), what
        # -- against the oracle
        orun = oracle.plan(inp, oracle.OracleTables.from_coordinate_system(co, obs), lo, hi, want_states=True, nthreads=4)
        out, status, cost, states, _ = fix
        np.testing.assert_array_equal(status & 3, orun.status & 3, err_msg=what)
        np.testing.assert_array_equal((status >> 4) & 7, (orun.status >> 4) & 7, err_msg=what)
        kin = (orun.status & 3) == 2
        np.testing.assert_array_equal((status >> 8)[kin], (orun.status >> 8)[kin], err_msg=what)
        has = ~np.isnan(orun.cost)
        assert np.all(np.isnan(cost[~has])), what
        np.testing.assert_allclose(cost[has], orun.cost[has], rtol=COST_RTOL, err_msg=what)
        lab = orun.status & 3
        defined = np.ones_like(has) if mode == "draw" else ((lab == 1) | (lab == 3))
        np.testing.assert_allclose(states[defined], orun.states[defined], rtol=0, atol=STATE_ATOL, err_msg=what)
        assert out.best_index == orun.out.best_index and out.n_feasible == orun.out.n_feasible and out.n_collision == orun.out.n_collision, what
        if orun.out.best_index >= 0:
            np.testing.assert_allclose(out.best_cost, orun.out.best_cost, rtol=COST_RTOL, err_msg=what)
            np.testing.assert_allclose(out.best_states, orun.out.best_states, rtol=0, atol=STATE_ATOL, err_msg=what)
        defined_rows += int(defined.sum())
        finite += int(has.sum())
        collided += int((lab == 3).sum())
        trajs = np.asarray(inp.traj_len)[(np.arange(lo, hi) // (len(inp.L) * len(inp.D)))]
        extended += int((trajs[defined] < n_steps).sum())
    # what was compared: a batch that stops holding finite costs, collisions or extended horizons fails instead of passing empty
    print(f"N + 1 = {n_steps}, {layout}: {defined_rows} state blocks, {finite} finite costs, {collided} collisions, {extended} extended blocks compared")
    # (the smallest counts over the horizons, from the oracle: 57 246 / 15 228 / 10 152 / 37 866 at N + 1 = 17)
    assert defined_rows >= 50000 and finite >= 15000 and collided >= 10000 and extended >= 35000
