"""Bit-identity of the three evaluation kernels: rp_eval_kernel with 16 lanes per candidate, rp_cost_kernel and
rp_chunk_kernel judge a candidate with the same status word and the same cost BITS.  This module holds what
tests/test_kernel_bit_identity.py needs: the kernel selections (options of a context), the comparison -- integers and uint64 views,
no tolerance anywhere --, the hand-built edge cases and the random ones.  No oracle: the kernels are compared with each other.

The other launch variants of rp_eval_kernel (32 / 64 lanes per candidate, the single-launch variant) add the same per-step terms in
another order: they are held to the bound of two summation orders of n non-negative doubles, summation_bound().

usage (GPU box): python tests/_bitid.py [first_seed] [n_cases]      random cases beyond the range the test module takes"""
import dataclasses
import functools
import math
import os
import sys

import numpy as np

if __name__ == "__main__":   # (as a script: the paths tests/conftest.py sets up for the suite)
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_repo, os.path.join(_repo, "commonroad-reactive-planner_amd"), os.path.join(_repo, "tests")]

from _lazy import lazy_relaxed

from commonroad_rp_amd import workloads as W
from commonroad_rp_amd._capi import (PlanInputs, make_params, make_cost, copy_params, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL,
                                     FLAG_SKIP_COLLISION, COST_DEFAULT, COST_FAILSAFE, LON_STOPPING, LON_VELOCITY_KEEPING)
from commonroad_rp_amd.collision import ObstacleTables
from commonroad_rp_amd.coordinate_system import CoordinateSystem

# ---- kernel selections ----------------------------------------------------------------------------------------------------------
# options every selection of the contract runs under: two-kernel path (the lane kernels read rp_lon_kernel's profile rows), no state
# rows, 16 lanes per candidate
BASE_OPTIONS = {"fused_lon": 0, "auto_materialize": 0, "lanes": 16}
# name -> (options, the kernel rp_last_kernel must name afterwards)
SELECTIONS = {
    "eval16": ({"cost_kernel": 0, "chunk_kernel": 0, "eval_block": 0}, "rp_eval_kernel"),
    "eval16_wave_wg": ({"cost_kernel": 0, "chunk_kernel": 0, "eval_block": 64}, "rp_eval_kernel"),   # one wavefront per workgroup
    "lane": ({"cost_kernel": 1, "chunk_kernel": 0, "eval_block": 0}, "rp_cost_kernel"),
    "chunk": ({"chunk_kernel": 1, "cost_kernel": 0, "eval_block": 0}, "rp_chunk_kernel"),
}
PASS1_KERNELS = ("eval16", "lane", "chunk")   # who computes the costs of the cost-ordered stage
# launch variants OUTSIDE the contract (another order of the additions): options on top of the context's defaults; None = default
BOUND_VARIANTS = {
    "g32": {"fused_lon": 0, "lanes": 32, "auto_materialize": 0},
    "g64": {"fused_lon": 0, "lanes": 64, "auto_materialize": 0},
    "single_launch": {"fused_lon": None, "lanes": None, "auto_materialize": None},
}
CHUNK_MIN_STEPS, CHUNK_MAX_STEPS = 17, 112   # rp_chunk_kernel: two to seven step blocks of 16 (csrc/rp_kernels.h, RP_CHUNK_MAX_BLOCKS)


def chunk_applies(N):
    return CHUNK_MIN_STEPS <= N + 1 <= CHUNK_MAX_STEPS


def selections_for(N):
    return [k for k in SELECTIONS if k != "chunk" or chunk_applies(N)]


def pass1_kernels_for(N):
    return [k for k in PASS1_KERNELS if k != "chunk" or chunk_applies(N)]


def summation_bound(N):
    """Two orders of adding the n = N + 1 per-step terms of a cost (the step loops of csrc/rp_kernels.h run i = 0 .. N, one term per
    step, the terminal and mid-horizon terms inside their step's) -- all of them non-negative -- each stay within (n - 1) 2^-53 of the
    exact sum, relative; so they differ by at most 2 (n - 1) 2^-53 relative."""
    return 2.0 * N * 2.0 ** -53


# ---- the comparison --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Run:
    status: np.ndarray
    cost: np.ndarray
    out: object      # PlanOutput
    kernel: str = ""
    path: int = 0


OUT_FIELDS = ("best_index", "best_cost", "n_feasible", "n_collision", "n_collision_before_best", "reason_counts")
OUT_FIELDS_COST_ORDERED = ("best_index", "best_cost", "n_feasible", "n_collision_before_best")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def status_cost_differences(st_a, cs_a, st_b, cs_b):
    """Every way two (status, cost) results can differ, as text; empty when they are the same integers and the same bits.  NaN costs
    (candidates without a cost) are equal to each other whatever their payload; a NaN on one side only is a difference."""
    st_a, st_b = np.asarray(st_a), np.asarray(st_b)
    cs_a, cs_b = np.asarray(cs_a, dtype=np.float64), np.asarray(cs_b, dtype=np.float64)
    if st_a.shape != st_b.shape or cs_a.shape != cs_b.shape or st_a.shape != cs_a.shape:
        return [f"shapes differ: status {st_a.shape} / {st_b.shape}, cost {cs_a.shape} / {cs_b.shape}"]
    found = []
    bad = np.flatnonzero(st_a.astype(np.int64) != st_b.astype(np.int64))
    if len(bad):
        i = int(bad[0])
        found.append(f"{len(bad)} status words differ, first at {i}: {int(st_a[i]):#x} (label {int(st_a[i]) & 3} reason {(int(st_a[i]) >> 4) & 7} "
                     f"step {int(st_a[i]) >> 8}) / {int(st_b[i]):#x} (label {int(st_b[i]) & 3} reason {(int(st_b[i]) >> 4) & 7} step {int(st_b[i]) >> 8})")
    na, nb = np.isnan(cs_a), np.isnan(cs_b)
    bad = np.flatnonzero(na != nb)
    if len(bad):
        i = int(bad[0])
        found.append(f"{len(bad)} costs are NaN on one side only, first at {i}: {cs_a[i]!r} / {cs_b[i]!r}")
    both = ~na & ~nb
    ba, bb = _bits(cs_a), _bits(cs_b)
    bad = np.flatnonzero(both & (ba != bb))
    if len(bad):
        i = int(bad[0])
        ulps = np.abs(ba[bad].astype(np.int64) - bb[bad].astype(np.int64))   # (finite costs are non-negative: the bit patterns are ordered)
        found.append(f"{len(bad)} finite costs differ in their bits (up to {int(ulps.max())} ulp), first at {i}: {cs_a[i]!r} {int(ba[i]):#018x} / "
                     f"{cs_b[i]!r} {int(bb[i]):#018x}")
    return found


def output_differences(a, b, fields=OUT_FIELDS):
    found = []
    for f in fields:
        va, vb = getattr(a, f), getattr(b, f)
        if f == "best_cost":
            same = (math.isnan(va) and math.isnan(vb)) or _bits([va])[0] == _bits([vb])[0]
        elif f == "reason_counts":
            same = np.array_equal(np.asarray(va), np.asarray(vb))
        else:
            same = int(va) == int(vb)
        if not same:
            found.append(f"{f}: {va!r} / {vb!r}" + (f" (bits {int(_bits([va])[0]):#018x} / {int(_bits([vb])[0]):#018x})" if f == "best_cost" else ""))
    return found


def bound_differences(a: Run, b: Run, N, rel=None):
    """A launch variant outside the bit-identity contract against eval16: status words exact, costs within summation_bound(N)
    relative (or `rel`)."""
    # (status words and NaN pattern as in the contract; the finite costs are masked out of that comparison and bounded below)
    found = status_cost_differences(a.status, np.where(np.isnan(a.cost), np.nan, 0.0), b.status, np.where(np.isnan(b.cost), np.nan, 0.0))
    both = ~np.isnan(a.cost) & ~np.isnan(b.cost)
    worst = 0.0
    if both.any():
        ca, cb = a.cost[both], b.cost[both]
        scale = np.maximum(np.abs(ca), np.abs(cb))
        dev = np.where(scale > 0, np.abs(ca - cb) / np.where(scale > 0, scale, 1.0), 0.0)
        worst = float(dev.max())
        lim = summation_bound(N) if rel is None else rel
        if not worst <= lim:
            i = int(np.flatnonzero(both)[int(np.argmax(dev))])
            found.append(f"cost of candidate {i} deviates {worst:.3g} relative, bound {lim:.3g} (n = {N + 1} steps): {a.cost[i]!r} / {b.cost[i]!r}")
    return found, worst


# ---- running one selection on a context ------------------------------------------------------------------------------------------
_VARIANT_KEYS = ("fused_lon", "auto_materialize", "lanes")


def new_context(device=0):
    from commonroad_rp_amd._capi import RpContext
    ctx = RpContext(device)
    ctx._bitid_defaults = {k: ctx.get_option(k) for k in _VARIANT_KEYS}   # (what rp_create gave: the single-launch variant runs on them)
    return ctx


def _set(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, ctx._bitid_defaults[k] if v is None else v)


def run_selection(ctx, inp, name, lo=0, hi=-1, lazy=0, sweep=0):
    """One plan of `inp` by the kernel selection `name`; the kernel that evaluated the batch must be the one asked for."""
    opts, kernel = SELECTIONS[name]
    _set(ctx, BASE_OPTIONS)
    _set(ctx, opts)
    _set(ctx, {"lazy": lazy, "sweep": sweep})
    out = ctx.plan(inp, lo, hi)
    got = ctx.last_kernel()
    assert got == kernel, f"selection {name}: the batch was evaluated by {got}, not by {kernel}"
    st, cs = ctx.fetch_status()
    return Run(st, cs, out, got, ctx.last_path())


def run_variant(ctx, inp, name, lo=0, hi=-1):
    _set(ctx, BOUND_VARIANTS[name])
    _set(ctx, {"cost_kernel": 0, "chunk_kernel": 0, "eval_block": 0, "lazy": 0, "sweep": 0})
    out = ctx.plan(inp, lo, hi)
    assert ctx.last_kernel() == "rp_eval_kernel" and ctx.last_path() == 0, (name, ctx.last_kernel(), ctx.last_path())
    st, cs = ctx.fetch_status()
    return Run(st, cs, out, ctx.last_kernel(), 0)


def production(inp, extra_flags=0):
    """`inp` as a production-mode plan: no FLAG_DRAW_ALL, no FLAG_MATERIALIZE_ALL (the lane kernels serve neither)."""
    p = copy_params(inp.params)
    p.flags = (p.flags & ~(FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)) | extra_flags
    return PlanInputs(p, inp.cost, inp.T, inp.traj_len, inp.L, inp.D)


def compare_kernels(ctx, inp, lo=0, hi=-1, what=""):
    """Eager comparison (every colliding candidate carries its label): every applicable selection against eval16.
    Returns eval16's run and the number of finite costs that were compared with each other kernel."""
    N = inp.params.N
    ref = run_selection(ctx, inp, "eval16", lo, hi)
    assert ref.path == 0, (what, ref.path)
    compared = {}
    for name in selections_for(N)[1:]:
        run = run_selection(ctx, inp, name, lo, hi)
        assert run.path == 0, (what, name, run.path)
        found = status_cost_differences(ref.status, ref.cost, run.status, run.cost) + output_differences(ref.out, run.out)
        assert not found, f"{what}: eval16 / {name} (N + 1 = {N + 1}, {len(ref.status)} candidates): " + "; ".join(found)
        compared[name] = int((~np.isnan(ref.cost)).sum())
    return ref, compared


def compare_cost_ordered(ctx, inp, eager: Run, lo=0, hi=-1, what=""):
    """The cost-ordered collision stage (list rounds, then the bounded sweep) with pass 1 by each kernel: the winner, its cost bits and
    the counters in front of it are the eager eval16 plan's; labels may be missing behind the winner only (_lazy.lazy_relaxed)."""
    N = inp.params.N
    paths = []
    for sweep in (0, 1):
        for name in pass1_kernels_for(N):
            run = run_selection(ctx, inp, name, lo, hi, lazy=1, sweep=sweep)
            tag = f"{what}: cost-ordered{' sweep' if sweep else ''}, pass 1 by {name} (path {run.path}) / eager eval16"
            if sweep:
                assert run.path == 3, tag
            else:
                assert run.path in (1, 2), tag
            found = output_differences(eager.out, run.out, OUT_FIELDS_COST_ORDERED)
            assert not found, tag + ": " + "; ".join(found)
            fixed, _ = lazy_relaxed(run.status, run.cost, eager, ctx, run.out, lo)
            found = status_cost_differences(eager.status, eager.cost, fixed, run.cost)
            assert not found, tag + ": " + "; ".join(found)
            paths.append(run.path)
    return paths


# ---- hand-built edge cases -------------------------------------------------------------------------------------------------------
DT = 0.1
STARTS = ("standstill_0", "standstill_002", "stopping", "lateral")
OBSTACLES = ("skip_flag", "none", "dynamic", "dynamic_70", "dynamic_short_table", "static")
MASKS = (31, 0, 5, 26)
FACTORS = (1, 2, 3)
COSTS = ("failsafe", "speed", "s", "plain", "speed_and_s")
CHUNK_HORIZONS = (17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 112)     # N + 1: all three kernels
OTHER_HORIZONS = (2, 3, 16, 113, 128, 130, 1001)                   # N + 1: eval16 and lane only


@dataclasses.dataclass(frozen=True)
class EdgeSpec:
    n_steps: int
    low: bool
    start: str
    obstacles: str
    mask: int
    factor: int
    cost: str

    @property
    def id(self):
        return f"n{self.n_steps}-{'lv' if self.low else 'hv'}-{self.start}-{self.obstacles}-m{self.mask}-f{self.factor}-{self.cost}"


def edge_matrix(horizons=CHUNK_HORIZONS):
    """One case per horizon and velocity mode; the other axes rotate through their values, so that every value of every axis meets both
    modes (test_edge_matrix_covers_every_axis: checked without a GPU) and -- every case runs every applicable kernel -- every kernel."""
    specs = []
    for low in (False, True):
        for i, n in enumerate(horizons):
            j = i + (3 if low else 0)
            specs.append(EdgeSpec(n, low, STARTS[j % 4], OBSTACLES[(j + j // 6) % 6], MASKS[(j // 2) % 4], FACTORS[(j // 3) % 3], COSTS[j % 5]))
    return specs


def traj_len_grid(n_steps):
    """First extended steps 16 k - 1, 16 k, 16 k + 1, 16 k + 2 for every step block k of the horizon -- the extension begins on the last
    lane of a block, on the first of the next, one step in -- and n_steps (no extension), in ONE batch."""
    tl = {n_steps}
    for k in range(1, (n_steps + 15) // 16 + 1):
        tl |= {16 * k - 1, 16 * k, 16 * k + 1, 16 * k + 2}
    tl = sorted(t for t in tl if 3 <= t <= n_steps)
    return tl or list(range(2, n_steps + 1))


def _route(length):
    s = np.arange(0.0, length, 1.0)
    return np.stack((s, 25.0 * np.sin(s / 70.0)), axis=1)


def _traffic(co, n_dyn, n_steps, s_lo, s_hi, step_dt, seed):
    """n_dyn constant-velocity boxes on and beside the route between s_lo and s_hi (some appear late or vanish early)."""
    rng = np.random.default_rng(seed)
    dyn = np.full((n_dyn, n_steps, 5), np.nan)
    s_max = co.ref_pos[-1] - 2.0
    for j in range(n_dyn):
        s0, vel, off = rng.uniform(s_lo, s_hi), rng.uniform(-2.0, 8.0), rng.uniform(-6.0, 6.0)
        if j % 3:   # (most of them beside the corridor: some candidates stay free)
            off = math.copysign(rng.uniform(3.2, 7.0), off)
        k0, k1 = (0, n_steps) if j % 5 else (int(rng.integers(0, max(1, n_steps // 3))), int(rng.integers(n_steps // 2, n_steps + 1)))
        for k in range(k0, k1, 1):
            s = s0 + vel * step_dt * k
            if not (1.0 < s < s_max):
                continue
            x, y = co.convert_to_cartesian_coords(s, off)
            dyn[j, k] = (x, y, rng.uniform(-3.2, 3.2), rng.uniform(1.0, 3.0), rng.uniform(0.5, 1.2))
    return dyn


def edge_obstacles(co, kind, N, factor, t0, s_lo, s_hi, seed=3):
    if kind == "none":
        return ObstacleTables()
    steps = t0 + N * factor + 5
    if kind == "dynamic_short_table":   # the table ends inside the horizon
        steps = max(1, t0 + (N * factor) // 2)
    n_dyn = {"dynamic_70": 70, "static": 4}.get(kind, 12)   # (70: beyond the 63 bits of the (pair, step) mask)
    dyn = _traffic(co, n_dyn, min(steps, 400), s_lo, s_hi, DT / factor, seed)
    if steps > dyn.shape[1]:   # (long horizons: the obstacles are gone after 400 table steps)
        dyn = np.concatenate((dyn, np.full((n_dyn, steps - dyn.shape[1], 5), np.nan)), axis=1)
    if kind != "static":
        return ObstacleTables(dyn_obb=dyn, dyn_t0=0)
    rng = np.random.default_rng(seed + 1)
    boxes, tris, circs = [], [], []
    for k in range(30):
        x, y = co.convert_to_cartesian_coords(rng.uniform(s_lo, min(s_hi, co.ref_pos[-1] - 3.0)), rng.choice([-1, 1]) * rng.uniform(1.8, 5.0))
        boxes.append([x, y, rng.uniform(-3, 3), rng.uniform(0.3, 4.0), rng.uniform(0.05, 0.5)])
        if k < 8:
            tris.append([x + 1, y + 1, x + 2.5, y + 1.2, x + 1.5, y + 2.6])
        if k < 6:
            circs.append([x - 2.0, y + 1.0, rng.uniform(0.2, 0.7)])
    return ObstacleTables(static_obb=boxes, static_tri=tris, static_circ=circs, dyn_obb=dyn, dyn_t0=0)


def edge_case(spec: EdgeSpec, nL=5, nD=7, T_of=None, route=None, vehicle=None):
    """PlanInputs, coordinate system and obstacle tables of one edge case."""
    N = spec.n_steps - 1
    horizon = N * DT
    stopping = spec.start == "stopping"
    v0 = {"standstill_0": 0.0, "standstill_002": 0.02, "stopping": 3.0 if spec.low else 6.0}.get(spec.start, 1.5 if spec.low else 9.0)
    v_hi = v0 + 5.0
    co = CoordinateSystem(route if route is not None else _route(max(400.0, 120.0 + 1.25 * v_hi * horizon)))
    k0 = int(np.searchsorted(co.ref_pos, 30.0))
    s0 = float(co.ref_pos[k0])
    tl = traj_len_grid(spec.n_steps)
    T = np.array([DT * (t - 1) for t in tl]) if T_of is None else np.asarray(T_of, dtype=float)
    if stopping:   # target positions: the quintic comes to rest at T, i.e. at its last valid step (first, last or second lane of a block)
        L = s0 + np.linspace(0.35, 0.9, nL) * v0 * max(T.mean(), 1.0)
    else:
        L = np.linspace(max(0.0, v0 - 4.0), v_hi, nL)
    # (from a standstill only small lateral moves are drivable in high-velocity mode: d' = d_dot / s_dot)
    D = np.append(np.linspace(-2.5, 2.5, nD - 1) * (0.02 if spec.start.startswith("standstill") else 1.0) + 0.3, 0.3)
    x0_lat = [0.3, 0.0 if spec.start.startswith("standstill") else (0.02 if spec.low else 0.05), 0.0]
    if spec.start == "lateral":
        x0_lat = [0.3, 0.2, -0.05] if spec.low else [0.3, 0.9, -0.4]
    th0 = float(co.ref_theta[k0]) + (math.atan(x0_lat[1]) if spec.low else math.asin(min(0.5, x0_lat[1] / max(v0, 0.5))))
    t0 = 2 if spec.factor > 1 else 0
    flags = FLAG_SKIP_COLLISION if spec.obstacles == "skip_flag" else 0
    veh = dict(W.VEHICLE2 if vehicle is None else vehicle)
    params = make_params(dt=DT, N=N, factor=spec.factor, time_step0=t0, low_vel_mode=spec.low, lon_mode=LON_STOPPING if stopping else LON_VELOCITY_KEEPING,
                         constraint_mask=spec.mask, flags=flags, x0_lon=[s0, v0, 0.1 if v0 > 0.5 else 0.0], x0_lat=x0_lat, x0_orientation=th0, **veh)
    if spec.cost == "failsafe":
        cost = make_cost(COST_FAILSAFE)
    else:
        cost = make_cost(COST_DEFAULT, w_a=1.0 if spec.cost == "s" else 5.0,
                         desired_speed=v0 + 1.0 if spec.cost in ("speed", "speed_and_s") else None, desired_d=0.5 if spec.cost == "plain" else 0.0,
                         desired_s=s0 + 20.0 if spec.cost in ("s", "speed_and_s") else None)
    obs = edge_obstacles(co, "dynamic" if spec.obstacles == "skip_flag" else spec.obstacles, N, spec.factor, t0, s0 - 5.0, s0 + 15.0 + v_hi * min(horizon, 12.0))
    return PlanInputs(params, cost, T, W.traj_len_of(T, DT), L, D), co, obs


def _bend_route(s_bend, s_end, kappa, ramp=15.0):
    """Straight up to s_bend, then the curvature rises linearly to `kappa` over `ramp` metres and stays; the route ENDS at s_end."""
    s = np.arange(0.0, s_end + 1e-9, 0.5)
    k = np.clip((s - s_bend) / ramp, 0.0, 1.0) * kappa
    th = np.cumsum(k * 0.5)
    return np.stack((np.cumsum(np.cos(th) * 0.5), np.cumsum(np.sin(th) * 0.5)), axis=1)


def failure_case(low, n_steps=65):
    """Candidates that fail a constraint or leave the projection domain at every step of the horizon's later blocks.  The route bends
    (left) with a curvature at the steering limit: samples on the inside of the bend (d > 0: kappa = k_r / (1 - k_r d)) exceed it at
    the step they get there, samples on the outside pass and run off the END of the route (out of domain at the step s passes it: the
    construction of tests/golden short_path_ood).  A fine grid of velocities spreads both over the steps."""
    spec = EdgeSpec(n_steps, low, "moving", "dynamic", 31, 1, "speed")
    k_bend = 0.025
    veh = dict(W.VEHICLE2, delta_max=math.atan(k_bend * W.VEHICLE2["wheelbase"]))
    N = n_steps - 1
    route = _bend_route(38.0, 50.0, k_bend, 8.0) if low else _bend_route(42.0, 59.0, k_bend)
    return edge_case(spec, nL=48, nD=7, T_of=[DT * 15, DT * 25, DT * N], route=route, vehicle=veh)


def block_edge_steps(status):
    """First failing steps (label 2) and first out-of-domain steps (reason 6) of a batch, as sets of step mod 16, from step 15 on."""
    st = np.asarray(status).astype(np.int64)
    step = st >> 8
    kin = ((st & 3) == 2) & (step >= 15)
    ood = (((st >> 4) & 7) == 6) & (step >= 15)
    return set((step[kin] % 16).tolist()), set((step[ood] % 16).tolist())


# ---- random cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_production_case(seed):
    """tests/_fuzz.py's case `seed` as a production-mode plan (FLAG_DRAW_ALL cleared: the lane kernels do not serve draw mode)."""
    from _fuzz import random_case
    inp, co, obs, info = random_case(seed)
    return production(inp), co, obs, info


def compare_random_case(ctx, seed):
    """Without the collision query and with the eager one, by every applicable kernel.  Returns (chunk ran, has a winner, finite costs compared)."""
    inp, co, obs, info = random_production_case(seed)
    ctx.set_coordinate_system(co)
    ctx.set_obstacles(obs)
    finite = 0
    winner = False
    chunk = False
    for extra in (FLAG_SKIP_COLLISION, 0):
        ref, compared = compare_kernels(ctx, production(inp, extra), what=f"seed {seed} {'no query' if extra else 'eager query'} {info}")
        finite += sum(compared.values())
        chunk = chunk or "chunk" in compared
        winner = winner or ref.out.best_index >= 0
    return chunk, winner, finite


def main(argv):
    first = int(argv[1]) if len(argv) > 1 else 100000
    n = int(argv[2]) if len(argv) > 2 else 1000
    ctx = new_context(0)
    chunk = winners = finite = bad = 0
    for seed in range(first, first + n):
        try:
            c, w, f = compare_random_case(ctx, seed)
        except AssertionError as e:
            bad += 1
            print(f"seed {seed}: {e}", flush=True)
            continue
        finally:
            random_production_case.cache_clear()
        chunk += c; winners += w; finite += f
    print(f"bit identity: {n} seeds from {first}, rp_chunk_kernel on {chunk}, {winners} with a winner, {finite} finite costs compared, {bad} seeds with differences")
    ctx.close()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
