"""The lean loop over the dynamic obstacles in rp_lon_kernel's broad phase (csrc/rp_kernels.h: near_mask_dyn_lean, option
"lean_broad") against the loop as it was ("lean_broad" = 0): the (pair, step) masks are the same bits, so status words, cost bits,
every element of every state row and the plan's result are the SAME BITS -- the lean loop changes how an obstacle's centre is
addressed, how a batch's radii are fetched and how its result bits are collected, not which obstacles get their bit.  Then every bit
position against the CPU oracle: one obstacle on the route, all others a kilometre away.

Everything goes through the C ABI on the two-kernel path ("fused_lon" = 0).  Which instance of rp_lon_kernel ran is read back
(read-only option "last_lon_lean") and asserted: a module that compares an instance with itself does not pass.

Shapes.  Obstacles per table 1, 7 (a tail only), 8, 16 (full batches of 8 only), 9, 17 (full + tail), 62, 63, 64, 65, 70 (the mask
has 63 bits of its own, bit 63 stands for the obstacles 63, 64, ...: the batch 56 .. 63 ends on it, the batch from 64 on is all
overflow, 65 and 70 have an overflow tail).  Horizons N + 1 = 17 (the 32-lane instance), 33 (64 lanes, half of them idle), 61, 64
(exactly one pass) and 65 (two passes, one live lane in the second).  Table steps per plan step 1 and 2.  Batches are a few hundred
candidates: 3 longitudinal x 7 lateral samples for every time sample of tests/_bitid.py: traj_len_grid."""
import functools

import numpy as np
import pytest

import _bitid as B
from _golden import Golden
from _paths import options
from commonroad_rp_amd._capi import PlanInputs, RpContext, copy_params, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL
from commonroad_rp_amd.collision import ObstacleTables

N_DYN = (1, 7, 8, 9, 16, 17, 62, 63, 64, 65, 70)
HORIZONS = (17, 33, 61, 64, 65)   # N + 1
FACTORS = (1, 2)
DRAW = FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL
N_LON, N_LAT = 3, 7
V0 = 9.0                          # tests/_bitid.py: edge_case, start "lateral" in high-velocity mode

# bit positions: obstacles per table -> the obstacle that stands on the route
LONE = {9: (0, 7, 8), 70: (0, 7, 8, 62, 63, 64, 69)}
LONE_STEPS = 61
LONE_AHEAD = 22.0                 # metres in front of the vehicle
FAR = 1000.0


def base_case(n_steps, factor):
    spec = B.EdgeSpec(n_steps, False, "lateral", "none", 31, factor, "speed")
    inp, co, _ = B.edge_case(spec, nL=N_LON, nD=N_LAT)
    return inp, co


def table_steps(inp):
    p = inp.params
    return p.time_step0 + p.N * p.factor + 5


@functools.lru_cache(maxsize=None)
def traffic_scene(n_steps, n_dyn, factor, short=False):
    """inputs, coordinate system and a table of n_dyn boxes in traffic (tests/_bitid.py: _traffic -- every fifth appears late or
    vanishes early, rows off the route are absent: NaN centres); short: the table ends inside the horizon"""
    inp, co = base_case(n_steps, factor)
    p = inp.params
    s0 = float(p.x0_lon[0])
    steps = max(1, p.time_step0 + (p.N * factor) // 2) if short else table_steps(inp)
    dyn = B._traffic(co, n_dyn, steps, s0 - 5.0, s0 + 15.0 + (V0 + 5.0) * min(p.N * B.DT, 12.0), B.DT / factor, 3 + n_dyn)
    return inp, co, ObstacleTables(dyn_obb=dyn, dyn_t0=0)


@functools.lru_cache(maxsize=None)
def folded_scene(n_steps):
    """7 dynamic rows and one small static rectangle beside the route: folded ("fold_static" = 1) it is the eighth row of a full batch"""
    inp, co, obs = traffic_scene(n_steps, 7, 1)
    s0 = float(inp.params.x0_lon[0])
    x, y = co.convert_to_cartesian_coords(s0 + 18.0, -2.4)
    return inp, co, ObstacleTables(static_obb=[[x, y, 0.3, 0.8, 0.4]], dyn_obb=obs.dyn_obb, dyn_t0=0)


@functools.lru_cache(maxsize=None)
def lone_scene(n_dyn, j):
    """obstacle j stands on the route ahead of the vehicle, every other one FAR away, at every step of the table"""
    inp, co = base_case(LONE_STEPS, 1)
    s0 = float(inp.params.x0_lon[0])
    steps = table_steps(inp)
    dyn = np.empty((n_dyn, steps, 5))
    for q in range(n_dyn):
        dyn[q, :] = (FAR + 7.0 * q, -FAR - 3.0 * q, 0.1 * q, 2.0, 0.9)
    k = int(np.searchsorted(co.ref_pos, s0 + LONE_AHEAD))
    x, y = co.convert_to_cartesian_coords(s0 + LONE_AHEAD, 0.3)
    dyn[j, :] = (x, y, float(co.ref_theta[k]), 2.0, 0.9)
    return inp, co, ObstacleTables(dyn_obb=dyn, dyn_t0=0)


def with_flags(inp, flags):
    p = copy_params(inp.params)
    p.flags = flags
    return PlanInputs(p, inp.cost, inp.T, inp.traj_len, inp.L, inp.D)


def lone_cases():
    return [(n, j) for n, js in LONE.items() for j in sorted(set(js + (n - 1,)))]


def test_lone_obstacle_scenes_decide_something():
    """without a GPU, the oracle alone: in every scene of the bit-position test at least one candidate collides and at least one is
    feasible -- a scene where nothing collides would pass with the obstacle's bit anywhere"""
    from oracle import oracle
    cases = lone_cases()
    assert set(cases) == {(9, 0), (9, 7), (9, 8), (70, 0), (70, 7), (70, 8), (70, 62), (70, 63), (70, 64), (70, 69)}
    labels = None
    for n_dyn, j in cases:
        inp, co, obs = lone_scene(n_dyn, j)
        inp = with_flags(inp, DRAW)
        run = oracle.plan(inp, oracle.OracleTables.from_coordinate_system(co, obs), 0, inp.n_candidates, want_states=False, nthreads=4)
        lab = run.status & 3
        assert (lab == 3).sum() >= 1 and (lab == 1).sum() >= 1, (n_dyn, j, np.bincount(lab, minlength=4))
        assert labels is None or np.array_equal(lab, labels), (n_dyn, j)   # (the same obstacle whatever its row: the same labels)
        labels = lab
    # the shapes of the bit-identity test: every way a table can fill the batches of 8 and the 63 + 1 bits
    assert {n % 8 for n in N_DYN} >= {0, 1, 7} and {62, 63, 64, 65} <= set(N_DYN) and min(N_DYN) < 8 < 64 < max(N_DYN)
    inp, _, obs = traffic_scene(61, 17, 1)
    assert inp.params.N == 60 and 100 <= inp.n_candidates <= 600 and np.isnan(obs.dyn_obb[:, :, 0]).any()


@pytest.fixture(scope="module")
def ctx():
    with options(fused_lon=0):
        c = RpContext(0)
        yield c
        c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(ctx, inp, lean, lo=0, hi=-1, states=True):
    ctx.set_option("lean_broad", lean)
    out = ctx.plan(inp, lo, hi)
    assert ctx.get_option("last_single_launch") == 0
    assert ctx.get_option("last_lon_lean") == lean, f"lean_broad = {lean}: the profile launch was the other instance"
    status, cost = ctx.fetch_status()
    return out, status, cost, ctx.fetch_states() if states else None


def compare_draw(ctx, inp, what, lo=0, hi=-1):
    """one draw-mode plan by each instance: status words, cost bits, state rows, result.  Returns (candidates, collisions)."""
    inp = with_flags(inp, DRAW)
    old = run(ctx, inp, 0, lo, hi)
    new = run(ctx, inp, 1, lo, hi)
    found = B.status_cost_differences(old[1], old[2], new[1], new[2]) + B.output_differences(old[0], new[0])
    assert not found, what + ": " + "; ".join(found)
    assert same_bits(old[3], new[3]), what + f": {int((old[3].view(np.uint64) != new[3].view(np.uint64)).sum())} state elements differ"
    if old[0].best_index >= 0:
        assert same_bits(old[0].best_states, new[0].best_states), what
    return len(new[1]), int(((new[1] & 3) == 3).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", HORIZONS)
def test_lean_loop_builds_the_same_masks(ctx, n_steps):
    ctx.set_option("lazy", -1)
    ctx.set_option("fold_static", -1)
    candidates = collisions = 0
    for factor in FACTORS:
        for n_dyn in N_DYN:
            inp, co, obs = traffic_scene(n_steps, n_dyn, factor)
            ctx.set_coordinate_system(co)
            ctx.set_obstacles(obs)
            n, c = compare_draw(ctx, inp, f"N + 1 = {n_steps}, {n_dyn} obstacles, factor {factor}")
            candidates += n
            collisions += c
    # the table ends inside the horizon: full batches, full + tail, overflow
    for n_dyn in (8, 17, 70):
        inp, co, obs = traffic_scene(n_steps, n_dyn, 2, True)
        assert obs.dyn_obb.shape[1] < inp.params.time_step0 + inp.params.N * 2
        ctx.set_coordinate_system(co)
        ctx.set_obstacles(obs)
        compare_draw(ctx, inp, f"N + 1 = {n_steps}, {n_dyn} obstacles, short table")
    # a range of candidates that begins and ends inside a (T, longitudinal sample) pair
    inp, co, obs = traffic_scene(n_steps, 17, 1)
    ctx.set_coordinate_system(co)
    ctx.set_obstacles(obs)
    lo, hi = N_LAT + 3, inp.n_candidates - 2 * N_LAT - 2
    assert lo % N_LAT and hi % N_LAT
    compare_draw(ctx, inp, f"N + 1 = {n_steps}, range [{lo}, {hi})", lo, hi)
    print(f"N + 1 = {n_steps}: {candidates} candidates, {collisions} of them colliding, compared bit for bit")
    assert collisions >= 100 and candidates - collisions >= 100   # (the masks decide something)


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", (61, 65))
def test_folded_rectangle_is_the_eighth_row(ctx, n_steps):
    inp, co, obs = folded_scene(n_steps)
    ctx.set_coordinate_system(co)
    ctx.set_obstacles(obs)
    ctx.set_option("lazy", -1)
    ctx.set_option("fold_static", 1)
    try:
        compare_draw(ctx, inp, f"N + 1 = {n_steps}, 7 dynamic rows + 1 folded rectangle")
        assert ctx.get_option("last_collision_level") == 1   # (folded: no static-shape query)
    finally:
        ctx.set_option("fold_static", -1)


@pytest.mark.gpu
def test_cost_ordered_production_plan(ctx):
    """production mode on the cost-ordered path ("lazy" = 1): winner, its cost bits and the counters in front of it"""
    ctx.set_option("fold_static", -1)
    ctx.set_option("lazy", 1)
    ctx.set_option("auto_materialize", 0)
    try:
        for n_dyn in (9, 70):
            inp, co, obs = traffic_scene(61, n_dyn, 1)
            ctx.set_coordinate_system(co)
            ctx.set_obstacles(obs)
            inp = with_flags(inp, 0)
            old = run(ctx, inp, 0, states=False)
            path = ctx.last_path()
            new = run(ctx, inp, 1, states=False)
            assert path in (1, 2, 3) and ctx.last_path() == path, (path, ctx.last_path())
            found = B.output_differences(old[0], new[0], B.OUT_FIELDS_COST_ORDERED) + B.status_cost_differences(old[1], old[2], new[1], new[2])
            assert not found, f"{n_dyn} obstacles, cost-ordered: " + "; ".join(found)
            if old[0].best_index >= 0:
                assert same_bits(old[0].best_states, new[0].best_states)
    finally:
        ctx.set_option("lazy", -1)
        ctx.set_option("auto_materialize", 1)


@pytest.mark.gpu
def test_explicit_polynomials_build_no_masks(ctx):
    """rp_plan_coeffs: the profile launch builds no masks, whichever instance it is"""
    g = Golden("arc_hv_l2_obs")
    g.setup_context(ctx)
    ctx.set_option("lazy", 0)
    try:
        n_ld = len(g.inputs.L) * len(g.inputs.D)
        tl, lon_t = np.repeat(g.inputs.traj_len, n_ld), np.repeat(g.inputs.T, n_ld)
        res = []
        for lean in (0, 1):
            ctx.set_option("lean_broad", lean)
            out = ctx.plan_coeffs(g.inputs.params, g.inputs.cost, g["lon_coeffs"], g["lat_coeffs"], lon_t, tl)
            assert ctx.get_option("last_lon_lean") == lean and ctx.get_option("last_single_launch") == 0
            res.append((out,) + tuple(ctx.fetch_status()))
        found = B.status_cost_differences(res[0][1], res[0][2], res[1][1], res[1][2]) + B.output_differences(res[0][0], res[1][0])
        assert not found, "; ".join(found)
        assert res[1][0].best_index == int(g["winner"]) and same_bits(res[0][0].best_states, res[1][0].best_states)
    finally:
        ctx.set_option("lazy", -1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_dyn", sorted(LONE))
def test_every_bit_position_lands_where_it_belongs(ctx, n_dyn):
    from oracle import oracle
    ctx.set_option("lazy", -1)
    ctx.set_option("fold_static", -1)
    for n, j in lone_cases():
        if n != n_dyn:
            continue
        inp, co, obs = lone_scene(n_dyn, j)
        inp = with_flags(inp, DRAW)
        ctx.set_coordinate_system(co)
        ctx.set_obstacles(obs)
        _, status, cost, _ = run(ctx, inp, 1, states=False)
        orun = oracle.plan(inp, oracle.OracleTables.from_coordinate_system(co, obs), 0, inp.n_candidates, want_states=False, nthreads=4)
        what = f"{n_dyn} obstacles, number {j} on the route"
        np.testing.assert_array_equal(status & 3, orun.status & 3, err_msg=what)
        np.testing.assert_array_equal((status >> 4) & 7, (orun.status >> 4) & 7, err_msg=what)
        assert ((status & 3) == 3).sum() >= 1, what
