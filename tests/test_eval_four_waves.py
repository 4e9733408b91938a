"""The four-wave instance of rp_eval_kernel's fixed-stride variant (csrc/rp_kernels.h: W4 -- compiled for four wavefronts per SIMD,
128 vector registers: the coefficients of the atan / sincos polynomials as scalar operands, rp_math.h) against the three-wave
instance of the same variant, pinned with the option "eval_waves" = 4 and 3: status words, cost bits and every element of every
state row are the SAME BITS -- the instance changes where constants live, not what is computed.  Then both against the CPU oracle at
the tolerances of tests/test_gpu_parity.py (one oracle run per plan; the two results are held to it one after the other).

Everything goes through the C ABI on the two-kernel path with 16 lanes per candidate.  Which instance evaluated a batch is read back
(read-only option "last_eval_waves") and asserted: a module that compares an instance with itself does not pass.

Shapes, as in tests/test_lean_step_block.py.  N + 1 = 61 and 64 have rows of 64 doubles under the default layout (last step block
partial / full); N + 1 = 49 takes the fixed-stride variant with the layout option "tail_split" = 0 (49 steps padded to 64).
N + 1 = 33 and 101 never have rows of 64 doubles: with "eval_waves" = 4 they must still run the generic code, report
"last_eval_waves" = 3 and pass.  Batches are ranges of 37 candidates and of 4 099 (37 lateral samples per pair), starting at
candidate 5 behind a multiple of 16.  The time samples (tests/_bitid.py: traj_len_grid) put the last valid step on the last lane of
a step block, on the first lane of the next, one and two lanes in, and hold L = N + 1.  Collision levels none / dynamic / static,
the four has_speed / has_s cost variants, draw and materialise modes and both batch sizes in full; the workgroup size (256 / 64
threads) and the low-velocity mode rotate against them, each meeting every value of the other axes."""
import functools

import numpy as np
import pytest

import _bitid as B
from _paths import options
from commonroad_rp_amd._capi import (PlanInputs, RpContext, RpError, copy_params, make_cost, COST_DEFAULT, FLAG_DRAW_ALL,
                                     FLAG_MATERIALIZE_ALL)

STATE_ATOL = 1e-6    # tests/test_gpu_parity.py
COST_RTOL = 1e-9

# (N + 1, layout): the three that take the fixed-stride variant, the two that never do
CASES = ((61, "default"), (64, "default"), (49, "unsplit"), (33, "default"), (101, "default"))
LAYOUTS = {"default": {"tail_split": 1}, "unsplit": {"tail_split": 0}}
FIXED = {(61, "default"), (64, "default"), (49, "unsplit")}
SIZES = (37, 4099)
FIRST = 5
N_LATERAL = 37
COLLISION = ("none", "dynamic", "static")
COSTS = {"plain": (False, False), "speed": (True, False), "s": (False, True), "speed_and_s": (True, True)}   # has_speed, has_s
MODES = {"draw": FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL, "materialise": FLAG_MATERIALIZE_ALL}
BLOCKS = (256, 64)
TWO_KERNEL_16 = {"fused_lon": 0, "lanes": 16}


def row_stride(n_steps, layout):
    """doubles between the state rows of the two-kernel path with 16 lanes per candidate (csrc/rp_host.hip: state_layout)"""
    r = n_steps % 16
    if layout == "default" and 0 < r <= 8 and n_steps - r >= 16:
        return n_steps - r   # split tail
    return (n_steps + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def scene(n_steps, collision, low):
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
    """(collision level, cost, mode, size, block, low-velocity mode) -- 48 plans per horizon"""
    out = []
    for ci, collision in enumerate(COLLISION):
        for k, cost in enumerate(COSTS):
            for mi, mode in enumerate(MODES):
                for si, size in enumerate(SIZES):
                    out.append((collision, cost, mode, size, BLOCKS[(ci + k + mi + si + n_steps) % 2], bool((k + (ci + si) // 2 + mi) % 2)))
    return out


def candidate_range(inp, size):
    lo = (inp.n_candidates // 2 if size < 100 else 0) // 16 * 16 + FIRST
    assert lo + size <= inp.n_candidates
    return lo, lo + size


def test_cases_are_what_they_claim():
    """without a GPU: the layouts the cases rely on, and that the combinations cover every axis at every collision level"""
    assert {c for c in CASES if row_stride(c[0], c[1]) == 64 and c[0] > 16} == FIXED
    for n, _ in CASES:
        cs = combos(n)
        assert len(set(cs)) == len(cs) == 48
        for axis, values in ((0, COLLISION), (1, COSTS), (2, MODES)):
            for v in values:
                mine = [c for c in cs if c[axis] == v]
                assert {c[3] for c in mine} == set(SIZES) and {c[4] for c in mine} == set(BLOCKS) and {c[5] for c in mine} == {False, True}
        tl = B.traj_len_grid(n)
        assert n in tl and any(t % 16 == 0 for t in tl) and any((t - 1) % 16 not in (0, 15) for t in tl if t < n)
    inp, _, _ = scene(61, "none", False)
    assert inp.params.N == 60 and inp.n_candidates >= FIRST + 4099


@pytest.fixture(scope="module")
def ctx():
    with options(**TWO_KERNEL_16):
        c = RpContext(0)
        yield c
        c.close()


def run(ctx, inp, lo, hi, block, waves):
    ctx.set_option("eval_block", block)
    ctx.set_option("eval_waves", waves)
    out = ctx.plan(inp, lo, hi)
    assert ctx.last_kernel() == "rp_eval_kernel" and ctx.last_path() == 0
    status, cost = ctx.fetch_status()
    return out, status, cost, ctx.fetch_states(), ctx.get_option("last_eval_waves"), ctx.get_option("last_fixed_stride")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def hold_to_oracle(result, orun, mode, what):
    out, status, cost, states = result[:4]
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
    return defined, has, lab


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps,layout", CASES)
def test_four_wave_instance_is_the_three_wave_one_bit_for_bit(ctx, n_steps, layout):
    from oracle import oracle
    for k, v in LAYOUTS[layout].items():
        ctx.set_option(k, v)
    ctx.set_option("fixed_stride", 1)
    fixed = (n_steps, layout) in FIXED
    defined_rows = finite = collided = extended = 0
    try:
        for collision, cost_name, mode, size, block, low in combos(n_steps):
            what = f"N + 1 = {n_steps}, {layout} layout, {collision}, cost {cost_name}, {mode}, block {block}, {'low' if low else 'high'} velocity, {size} candidates"
            base, co, obs = scene(n_steps, collision, low)
            inp = with_cost_and_flags(base, cost_name, MODES[mode])
            ctx.set_coordinate_system(co)
            ctx.set_obstacles(obs)
            lo, hi = candidate_range(inp, size)
            w3 = run(ctx, inp, lo, hi, block, 3)
            w4 = run(ctx, inp, lo, hi, block, 4)
            assert w3[4] == 3 and w3[5] == int(fixed), what
            assert w4[4] == (4 if fixed else 3) and w4[5] == int(fixed), what   # the instance under test ran exactly where the variant applies
            assert len(w4[1]) == size and w4[3].shape == (size, 14, n_steps), what
            # -- bit for bit: status, cost, every state row; the plan's result
            found = B.status_cost_differences(w3[1], w3[2], w4[1], w4[2]) + B.output_differences(w3[0], w4[0])
            assert not found, what + ": " + "; ".join(found)
            assert same_bits(w3[3], w4[3]), what + f": {int((w3[3].view(np.uint64) != w4[3].view(np.uint64)).sum())} state elements differ"
            if w3[0].best_index >= 0:
                assert same_bits(w3[0].best_states, w4[0].best_states), what
            # -- both against the oracle
            orun = oracle.plan(inp, oracle.OracleTables.from_coordinate_system(co, obs), lo, hi, want_states=True, nthreads=4)
            hold_to_oracle(w3, orun, mode, what + ", three waves")
            defined, has, lab = hold_to_oracle(w4, orun, mode, what + ", four waves")
            defined_rows += int(defined.sum())
            finite += int(has.sum())
            collided += int((lab == 3).sum())
            trajs = np.asarray(inp.traj_len)[(np.arange(lo, hi) // (len(inp.L) * len(inp.D)))]
            extended += int((trajs[defined] < n_steps).sum())
    finally:
        ctx.set_option("eval_waves", 0)
        ctx.set_option("tail_split", 1)
    # what was compared: a batch that stops holding finite costs, collisions or extended horizons fails instead of passing empty
    # (bounds: the smallest counts over the horizons of tests/test_lean_step_block.py, which builds the same scenes)
    print(f"N + 1 = {n_steps}, {layout}: {defined_rows} state blocks, {finite} finite costs, {collided} collisions, {extended} extended blocks compared")
    assert defined_rows >= 50000 and finite >= 15000 and collided >= 10000 and extended >= 35000


@pytest.mark.gpu
def test_eval_waves_option(ctx):
    """3 and 4 are taken, 5 (and 1, 2, -1) refused with RP_EINVAL (-1) and the value kept, 0 restores the policy; "last_eval_waves" is
    read-only"""
    ctx.set_option("eval_waves", 0)
    for v in (3, 4):
        ctx.set_option("eval_waves", v)
        assert ctx.get_option("eval_waves") == v
    for bad in (5, 1, 2, -1):
        with pytest.raises(RpError, match=r"-> -1:"):
            ctx.set_option("eval_waves", bad)
        assert ctx.get_option("eval_waves") == 4
    with pytest.raises(RpError, match=r"-> -1:"):
        ctx.set_option("last_eval_waves", 4)
    ctx.set_option("eval_waves", 0)
    assert ctx.get_option("eval_waves") == 0
    # under the policy a fixed-stride plan reports one of the two instances, and its result is that instance's
    base, co, obs = scene(61, "dynamic", False)
    inp = with_cost_and_flags(base, "speed", MODES["draw"])
    ctx.set_coordinate_system(co)
    ctx.set_obstacles(obs)
    ctx.set_option("tail_split", 1)
    ctx.set_option("fixed_stride", 1)
    lo, hi = candidate_range(inp, 4099)
    by_policy = run(ctx, inp, lo, hi, 256, 0)
    assert by_policy[5] == 1 and by_policy[4] in (3, 4)
    pinned = run(ctx, inp, lo, hi, 256, by_policy[4])
    ctx.set_option("eval_waves", 0)
    assert pinned[4] == by_policy[4]
    assert not B.status_cost_differences(by_policy[1], by_policy[2], pinned[1], pinned[2]) and same_bits(by_policy[3], pinned[3])
