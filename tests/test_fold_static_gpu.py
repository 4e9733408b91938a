"""Static rectangles checked as rows of the dynamic-obstacle table (option "fold_static", csrc/rp_host.hip: fold_view): a plan with
"fold_static" = 1 against the same plan with "fold_static" = 0 -- status words, cost bits, every counter of the result and the
winner's state block must be the same integers and bits, on every launch path of tests/_paths.py and in draw, materialize and fused
mode -- and which of the two views a plan took (read-only option "last_collision_level": 2 unfolded, 1 folded).

Scenes: ZAM_Over-1_1 at sampling level 1 (one static rectangle, no dynamic obstacle) and DEU_Test-1_1_T-1 with cfg3's 49 synthetic
boxes on a 5 x 5 x 9 grid at N = 60 (one static rectangle in the ego lane, 50 dynamic obstacles)."""
import functools

import numpy as np
import pytest

import _bitid as B
from _paths import LAUNCH_PATHS, options
from commonroad_rp_amd import workloads as W
from commonroad_rp_amd._capi import FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL, PlanInputs, RpContext, copy_params
from commonroad_rp_amd.collision import ObstacleTables

MODES = {"draw": FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL, "materialize": FLAG_MATERIALIZE_ALL, "fused": 0}


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "over":
        return W.cfg1(level=1)
    dt = 0.1
    return W._scenario_workload("deu", "DEU_Test-1_1_T-1", 60, [dt * (30 + 4 * k) for k in range(5)], 9, 5, low_vel_threshold=4.0,
                                extra_obstacles=49, extra_lane=5.0)


def with_flags(inp, flags, time_step0=None):
    p = copy_params(inp.params)
    p.flags = (p.flags & ~(FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)) | flags
    if time_step0 is not None:
        p.time_step0 = time_step0
    return PlanInputs(p, inp.cost, inp.T, inp.traj_len, inp.L, inp.D)


def tables(w, **changes):
    ob = w.obstacles
    kw = dict(static_obb=ob.static_obb, static_tri=ob.static_tri, static_circ=ob.static_circ, dyn_obb=ob.dyn_obb, dyn_t0=ob.dyn_t0)
    kw.update(changes)
    return ObstacleTables(**kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(ctx, inp, fold, lo=0, hi=-1):
    ctx.set_option("fold_static", fold)
    out = ctx.plan(inp, lo, hi)
    status, cost = ctx.fetch_status()
    return out, status, cost, ctx.get_option("last_collision_level")


def differences(a, b):
    found = B.status_cost_differences(a[1], a[2], b[1], b[2]) + B.output_differences(a[0], b[0])
    if a[0].best_index >= 0 and b[0].best_index >= 0 and not same_bits(a[0].best_states, b[0].best_states):
        found.append("the winner's state block differs")
    return found


def assert_folded_equals_unfolded(ctx, inp, what, lo=0, hi=-1, levels=(2, 1)):
    off, on = run(ctx, inp, 0, lo, hi), run(ctx, inp, 1, lo, hi)
    assert (off[3], on[3]) == levels, what
    found = differences(off, on)
    assert not found, what + ": " + "; ".join(found)
    return off, on


def new_context(w, obstacles=None):
    ctx = RpContext(0)
    ctx.set_coordinate_system(w.coordinate_system)
    ctx.set_obstacles(obstacles if obstacles is not None else w.obstacles)
    return ctx


def test_scenes_are_what_they_claim():
    """without a GPU: one static rectangle each, no dynamic table | 50 dynamic obstacles none of which is smaller than the rectangle"""
    over, deu = scene("over"), scene("deu")
    assert len(over.obstacles.static_obb) == 1 and over.obstacles.dyn_obb.shape[0] * over.obstacles.dyn_obb.shape[1] == 0
    assert len(over.obstacles.static_tri) == 0 and len(over.obstacles.static_circ) == 0
    assert len(deu.obstacles.static_obb) == 1 and deu.obstacles.dyn_obb.shape[0] == 50 and deu.inputs.params.N == 60
    assert deu.inputs.n_candidates in (5 * 5 * 9, 5 * 6 * 9)
    r_static = np.hypot(*deu.obstacles.static_obb[0, 3:5])
    assert r_static <= np.nanmax(np.hypot(deu.obstacles.dyn_obb[..., 3], deu.obstacles.dyn_obb[..., 4]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(LAUNCH_PATHS))
def test_folded_plan_is_the_unfolded_plan(path):
    """static only (ZAM_Over) and static plus dynamic (DEU_Test + 49 boxes), every mode, on one launch path"""
    with options(**LAUNCH_PATHS[path]):
        for name in ("over", "deu"):
            w = scene(name)
            ctx = new_context(w)
            collided = 0
            for mode, flags in MODES.items():
                off, _ = assert_folded_equals_unfolded(ctx, with_flags(w.inputs, flags), f"{name}, {mode}, {path}")
                collided += off[0].n_collision
            assert collided > 0, f"{name}, {path}: no candidate collides, nothing was compared"
            ctx.close()


@pytest.mark.gpu
def test_static_rectangle_decides_labels():
    """the rectangle matters in both scenes: without it fewer candidates collide (so the folded row is what reports them)"""
    for name in ("over", "deu"):
        w = scene(name)
        ctx = new_context(w)
        inp = with_flags(w.inputs, MODES["draw"])
        with_rect = run(ctx, inp, 1)
        assert with_rect[3] == 1
        ctx.set_obstacles(tables(w, static_obb=np.zeros((0, 5))))
        without = run(ctx, inp, 1)
        assert without[3] == (1 if name == "deu" else 0)
        assert with_rect[0].n_collision > without[0].n_collision, name
        ctx.close()


@pytest.mark.gpu
def test_horizon_past_the_dynamic_window():
    """time_step0 such that the horizon runs out of, and then starts behind, the dynamic obstacles' window: they are absent there,
    the static rectangle still collides"""
    w = scene("deu")
    ob = w.obstacles
    n_steps = ob.dyn_obb.shape[1]
    ctx = new_context(w)
    for t0 in (ob.dyn_t0 + n_steps - 20, ob.dyn_t0 + n_steps + 3):
        for mode in ("draw", "fused"):
            off, on = assert_folded_equals_unfolded(ctx, with_flags(w.inputs, MODES[mode], time_step0=t0), f"time_step0 {t0}, {mode}")
            assert on[0].n_collision > 0
    # behind the window only the rectangle is left: the same labels as with the rectangle alone
    inp = with_flags(w.inputs, MODES["draw"], time_step0=ob.dyn_t0 + n_steps + 3)
    on = run(ctx, inp, 1)
    ctx.set_obstacles(tables(w, dyn_obb=None))
    alone = run(ctx, inp, 0)
    assert alone[3] == 2 and not differences(alone, on)
    ctx.close()


@pytest.mark.gpu
def test_second_plan_regrows_the_table():
    w = scene("deu")
    ob = w.obstacles
    ctx = new_context(w)
    first = with_flags(w.inputs, MODES["draw"])
    assert ctx.get_option("fold_static_steps") == 0
    assert_folded_equals_unfolded(ctx, first, "first plan")
    steps = ctx.get_option("fold_static_steps")
    assert steps >= max(ob.dyn_obb.shape[1], first.params.time_step0 - ob.dyn_t0 + 61)
    far = with_flags(w.inputs, MODES["draw"], time_step0=ob.dyn_t0 + steps + 40)    # every step beyond what the table covers
    assert_folded_equals_unfolded(ctx, far, "plan that reaches past the table")
    grown = ctx.get_option("fold_static_steps")
    assert grown >= steps + 40 + 61
    assert_folded_equals_unfolded(ctx, first, "first plan again")                  # (never shrinks; the dynamic rows are intact)
    assert ctx.get_option("fold_static_steps") == grown
    ctx.set_obstacles(ob)                                                          # new tables: built anew by the next folded plan
    assert ctx.get_option("fold_static_steps") == 0
    assert_folded_equals_unfolded(ctx, first, "after rp_set_obstacles")
    ctx.close()


@pytest.mark.gpu
def test_step_before_dyn_t0_keeps_the_unfolded_tables():
    w = scene("deu")
    ctx = new_context(w)
    inp = with_flags(w.inputs, MODES["draw"], time_step0=w.obstacles.dyn_t0 - 1)
    assert_folded_equals_unfolded(ctx, inp, "time_step0 = dyn_t0 - 1", levels=(2, 2))
    assert_folded_equals_unfolded(ctx, with_flags(w.inputs, MODES["draw"], time_step0=w.obstacles.dyn_t0), "time_step0 = dyn_t0")
    ctx.close()


@pytest.mark.gpu
def test_level_chain_over_a_folded_table():
    """rp_plan_levels over ZAM_Over's sampling levels 1 .. 3: one table for the chain, the result of the unfolded chain"""
    ws = [W.cfg1(level=k) for k in (1, 2, 3)]
    levels = [(w.inputs.T, w.inputs.traj_len, w.inputs.L, w.inputs.D) for w in ws]
    ctx = new_context(ws[0])
    got = {}
    for fold in (0, 1):
        ctx.set_option("fold_static", fold)
        ctx.plan_levels_begin(ws[0].inputs.params, ws[0].inputs.cost, levels)
        out = ctx.plan_wait()
        status, cost = ctx.fetch_status()
        got[fold] = (out, status, cost, ctx.get_option("last_collision_level"), ctx.last_level())
    assert (got[0][3], got[1][3]) == (2, 1) and got[0][4] == got[1][4]
    found = differences(got[0], got[1])
    assert not found, "; ".join(found)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["draw", "fused"])
def test_two_shards_against_the_unsharded_plan(mode):
    w = scene("deu")
    ctx = new_context(w)
    inp = with_flags(w.inputs, MODES[mode])
    n, half = inp.n_candidates, inp.n_candidates // 2 + 3
    whole_off, whole_on = assert_folded_equals_unfolded(ctx, inp, f"whole grid, {mode}")
    parts = [assert_folded_equals_unfolded(ctx, inp, f"shard [{lo}, {hi}), {mode}", lo, hi)[1] for lo, hi in ((0, half), (half, n))]
    status, cost = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    found = B.status_cost_differences(whole_off[1], whole_off[2], status, cost)
    assert not found, "; ".join(found)
    ctx.close()


@pytest.mark.gpu
def test_swept_check_reads_the_tables_as_uploaded():
    """after a folded plan rp_check_swept still rejects a pose inside the static rectangle (ZAM_Over: nothing else to collide with)"""
    w = scene("over")
    ctx = new_context(w)
    assert run(ctx, with_flags(w.inputs, MODES["draw"]), 1)[3] == 1
    cx, cy, th = w.obstacles.static_obb[0, :3]
    p = w.inputs.params
    assert ctx.check_swept(p, [cx, cx + 0.05 * np.cos(th)], [cy, cy + 0.05 * np.sin(th)], [th, th]) == 0
    assert ctx.check_swept(p, [cx + 500.0, cx + 500.05], [cy + 500.0, cy + 500.0], [0.0, 0.0]) == -1
    ctx.close()


def refused_tables():
    w = scene("deu")
    ob = w.obstacles
    rect = ob.static_obb[0]
    far = rect[:2] + 900.0
    more = np.tile(rect, (14, 1))
    more[:, 0] += 600.0 + 10.0 * np.arange(14)
    bad = np.concatenate((ob.static_obb, [[far[0], far[1], 0.0, np.inf, 1.0]]))
    return {
        "a triangle present": tables(w, static_tri=[[far[0], far[1], far[0] + 2.0, far[1], far[0], far[1] + 2.0]]),
        "a circle present": tables(w, static_circ=[[far[0], far[1], 1.0]]),
        "64 obstacles in total": tables(w, static_obb=more),
        "a rectangle larger than every dynamic obstacle": tables(w, static_obb=[[rect[0], rect[1], rect[2], 3.0, 1.0]]),
        "a non-finite row": tables(w, static_obb=bad),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a triangle present", "a circle present", "64 obstacles in total",
                                  "a rectangle larger than every dynamic obstacle", "a non-finite row"])
def test_tables_that_are_not_folded(case):
    w = scene("deu")
    ctx = new_context(w, refused_tables()[case])
    assert_folded_equals_unfolded(ctx, with_flags(w.inputs, MODES["draw"]), case, levels=(2, 2))
    ctx.close()


@pytest.mark.gpu
def test_rule_folds_few_rectangles_only():
    """"fold_static" = -1: up to four rectangles next to a dynamic table (csrc/rp_host.hip: kFoldMaxRects); rectangles alone are left
    to the grid"""
    over = scene("over")
    ctx = new_context(over)
    assert run(ctx, with_flags(over.inputs, MODES["draw"]), -1)[3] == 2
    ctx.close()
    w = scene("deu")
    rect = w.obstacles.static_obb[0]
    inp = with_flags(w.inputs, MODES["draw"])
    for k, level in ((1, 1), (4, 1), (5, 2)):
        rects = np.tile(rect, (k, 1))
        rects[:, 0] += 700.0 * np.arange(k)
        ctx = new_context(w, tables(w, static_obb=rects))
        assert run(ctx, inp, -1)[3] == level, k
        assert_folded_equals_unfolded(ctx, inp, f"{k} rectangles")
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["over", "deu"])
def test_nan_pose_collides_on_both_views(name):
    """A NaN in the reference's orientation table reaches the heading, and with it the centre of the ego rectangle, of candidates that
    are inside the projection domain and pass every constraint check: such a pose still asks.  The walk over static shapes reports a
    hit for it (none of its comparisons is true), and so must the folded view, whose circle tests alone would say "far"."""
    w = scene(name)
    # (the rectangle itself a kilometre away: whatever it adds to the collisions, it adds through the poses that are NaN)
    rect = w.obstacles.static_obb[0].copy()
    rect[:2] += 1000.0
    obstacles = tables(w, static_obb=[rect])
    co = w.coordinate_system
    theta = np.array(co.ref_theta, dtype=np.float64)
    s0 = float(w.inputs.params.x0_lon[0])
    hole = (np.asarray(co.ref_pos) > s0 + 12.0) & (np.asarray(co.ref_pos) < s0 + 18.0)
    assert hole.sum() >= 2
    theta[hole] = np.nan
    got = {}
    for label, th in (("clean", co.ref_theta), ("nan", theta)):
        ctx = RpContext(0)
        ctx.set_reference(co.ref_pos, th, co.ref_curv, co.ref_curv_d, co.reference, getattr(co, "proj_domain_d_limit", 20.0))
        ctx.set_obstacles(obstacles)
        for mode in ("draw", "fused"):
            off, on = assert_folded_equals_unfolded(ctx, with_flags(w.inputs, MODES[mode]), f"{name}, {label} reference, {mode}")
            got[label, mode] = off
        ctx.close()
    # (the case is what it claims: the NaN poses add collisions in draw mode, where every candidate is labelled)
    print(name, "collisions, clean reference", got["clean", "draw"][0].n_collision, "with NaN headings", got["nan", "draw"][0].n_collision)
    assert got["nan", "draw"][0].n_collision > got["clean", "draw"][0].n_collision
