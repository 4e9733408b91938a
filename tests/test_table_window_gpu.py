"""The reference-table window of the single-launch kernel on the device (csrc/rp_kernels.h, LON_FUSED prologue; the host rule is
csrc/rp_table_window.h).  Needs a real MI355X: ``pytest -m gpu``.

Every plan of this module runs on one context with default options, takes the single-launch variant ("last_single_launch" == 1) and
carries the window tests/_window.py computes for it ("last_table_window", "last_table_window_first").  It is compared three ways:

  (a) against the CPU oracle, with the tolerances of tests/test_gpu_parity.py (states 1e-6 absolute, costs 1e-9 relative; labels,
      reasons, steps, counters and the winner exact);
  (b) against the same plan with "table_window" = 0 on the same context, WITHOUT tolerance: status words, cost bits, every result
      counter, the winner's state block and, where the plan keeps them, all state rows as uint64 -- both sides run the same
      instructions on what should be the same LDS values;
  (c) after a poison plan: immediately before every windowed plan a second context on the same device plans a batch of the same
      launch shape (same grids, same obstacle tables, same flags) with "table_window" = 0 on a reference with the same vertex count
      whose every row differs (the path mirrored, turned and moved; its arclength compressed unevenly around the middle of the
      window, so that a stale vertex position misleads the lookup's fix-ups below the window as well as above it).  LDS is not cleared between workgroups: whatever earlier workgroups left at the table's offsets is then NOT the
      right table, and a read of an entry nobody staged shows up in (a) and (b).  This is a best effort: nothing forces a workgroup
      of the windowed plan onto a compute unit and an LDS allocation the poison plan used; on an idle device with launches of the
      same shape and size it is the likely placement, no more.

In every scene tests/_window.py classifies each workgroup on the CPU -- from the prologue's own item set: the pairs its
256 / lanes candidates touch, steps 0 .. N, valid or extrapolated -- as "no item outside the window" or "some item outside" (the
second kind copies the whole block and computes every item again); every item's s keeps 1e-6 m from win_s_lo and win_s_hi, so that
rounding cannot change the class; and the scene asserts the classes it is there for.

What this module sees and what it cannot (each changed library run once against it, DESIGN.md section 4, "Table window"): a second
pass that does not start its item loop again turns every scene red in which a VALID step lies outside the window (at_start, at_end,
stopping, ...).  Bounds one segment wider (win_s_hi = pos[w0 + wn - 3], win_s_lo = pos[w0 + 1], bucket range computed from them) stay
green, and rightly so: by tests/test_table_window_host.py such items still read staged entries only -- the vertex margins of a window
clamped at neither end have that much slack.  Rows of extrapolated steps (i >= traj_len) left uncomputed stay green as well: the
evaluation reads nothing of them but the broad-phase masks, which come from the last valid step.

Scene 8 of the list (a valid step in the FIRST admissible segment w0 + 2): tests/test_table_window_host.py::test_first_valid_segment
confirms that the rule reaches it only when w0 was clamped -- otherwise w0 = seg_lo - 3 and the first segment of a valid step is
w0 + 3; a window moved down by the clamp at the table's end starts even further below seg_lo -- i.e. only at the start of the
table, w0 == 0 with the plan starting in segment 2: `first_segment` below.
"""
import numpy as np
import pytest

import _window as W
from _bitid import edge_obstacles, output_differences, status_cost_differences
from commonroad_rp_amd._capi import (FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL, LON_STOPPING, LON_VELOCITY_KEEPING, PlanInputs, RpContext, copy_params,
                                     make_cost, make_params)
from commonroad_rp_amd.collision import ObstacleTables
from commonroad_rp_amd.coordinate_system import CoordinateSystem
from commonroad_rp_amd.workloads import VEHICLE2, traj_len_of
from test_gpu_parity import COST_RTOL, STATE_ATOL, _compare_collision_counts, _compare_out, _compare_status

pytestmark = pytest.mark.gpu

DT = 0.1
MARGIN = 1e-6   # metres between every classified item and the window's bounds


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def polyline(seg):
    """a gently winding polyline with the given segment lengths: its arclengths are their running sum"""
    seg = np.asarray(seg, dtype=np.float64)
    s = np.concatenate(([0.0], np.cumsum(seg)))
    th = 0.35 * np.sin(s[:-1] / 40.0)
    return np.concatenate((np.zeros((1, 2)), np.cumsum(np.stack((seg * np.cos(th), seg * np.sin(th)), axis=1), axis=0)))


class Scene:
    def __init__(self, seg, k0, v0, T, L, nD=7, N=30, a0=0.2, frac=0.5, low=False, stopping=False, obstacles="none", flags=0):
        """starts `frac` of the way into segment k0; L: target velocities, or (stopping) target positions RELATIVE to the start"""
        self.co = CoordinateSystem(polyline(seg))
        pos = self.co.ref_pos
        self.pos = np.asarray(pos, dtype=np.float64)
        self.s0 = float(pos[k0] + frac * (pos[k0 + 1] - pos[k0]))
        self.k0, self.N, self.nD = k0, N, nD
        self.mode = LON_STOPPING if stopping else LON_VELOCITY_KEEPING
        self.T = np.asarray(T, dtype=np.float64)
        self.L = np.asarray(L, dtype=np.float64) + (self.s0 if stopping else 0.0)
        self.D = np.append(np.linspace(-2.5, 2.5, nD - 1), 0.3)
        self.x0_lon = [self.s0, float(v0), float(a0)]
        self.params = make_params(dt=DT, N=N, x0_lon=self.x0_lon, x0_lat=[0.3, 0.05, 0.0], x0_orientation=float(self.co.ref_theta[k0]),
                                  low_vel_mode=low, lon_mode=self.mode, flags=flags, **VEHICLE2)
        self.cost = make_cost(desired_speed=8.0)
        self.obstacle_kind = obstacles
        self.obs = edge_obstacles(self.co, obstacles, N, 1, 0, max(2.0, self.s0 - 5.0), min(self.s0 + 15.0 + 3.0 * abs(v0), float(pos[-1]) - 3.0))
        self.bk = W.bucket_table(self.pos)
        self.window = W.rule_window(self.pos, self.bk, self.mode, self.x0_lon, self.T, self.L)

    def inputs(self, flags=None):
        p = copy_params(self.params)
        if flags is not None:
            p.flags = flags
        return PlanInputs(p, self.cost, self.T, traj_len_of(self.T, DT), self.L, self.D)

    @property
    def n_candidates(self):
        return len(self.T) * len(self.L) * self.nD

    def classes(self, lanes, cand_begin=0, n_cand=None):
        if self.window.n == 0:
            return None, None
        return W.classify(self.pos, self.window, self.mode, self.x0_lon, self.T, self.L, self.nD, self.N, DT, lanes, cand_begin, n_cand)

    def valid_positions(self):
        """s of the valid steps (i < traj_len) of every pair"""
        S = W.pair_positions(self.mode, self.x0_lon, self.T, self.L, self.N, DT)
        tl = np.repeat(traj_len_of(self.T, DT), len(self.L))
        return S, np.arange(self.N + 1)[None, :] < tl[:, None]

    def poison(self):
        """The reference of the poison plan -- same vertex count, every row different -- and the plan's inputs on it."""
        n = len(self.pos)
        k = np.arange(n - 1)
        seg = np.diff(self.pos) * 0.3 * (1.0 + 0.2 * np.sin(1.0 + 0.7 * k))
        xy = polyline(seg)
        c, s = np.cos(0.9), np.sin(0.9)
        xy = np.stack((c * xy[:, 0] + s * xy[:, 1], s * xy[:, 0] - c * xy[:, 1]), axis=1) + np.array([1000.0, -500.0])   # mirrored, turned, moved
        co = CoordinateSystem(xy)
        # its arclength: the path's, compressed unevenly to about 0.3 around the middle of the window -- a stale vertex position read
        # BELOW the window is then larger than the item's s and one read ABOVE it smaller: either way the opposite of what the fix-ups
        # of the lookup would have found in the right table
        w = self.window
        kc = int(np.searchsorted(self.pos, 0.5 * (w.s_lo + w.s_hi))) if w.n else self.k0
        kc = min(max(kc, 0), n - 1)
        ppos = np.asarray(co.ref_pos)
        ppos = ppos - ppos[kc] + self.pos[kc] + 0.123
        tables = (ppos, np.asarray(co.ref_theta) + 0.7, np.asarray(co.ref_curv) + 0.013, np.asarray(co.ref_curv_d) + 0.0007, np.asarray(co.reference))
        assert len(tables[0]) == n
        own = (self.pos, self.co.ref_theta, self.co.ref_curv, self.co.ref_curv_d, np.asarray(self.co.reference)[:, 0], np.asarray(self.co.reference)[:, 1])
        for a, b in zip(own, tables[:4] + (tables[4][:, 0], tables[4][:, 1])):
            assert np.all(np.asarray(a) != np.asarray(b))
        assert np.all(np.diff(self.pos) != np.diff(tables[0]))   # (the reciprocal segment lengths)
        s0 = float(tables[0][self.k0] + 0.5 * (tables[0][self.k0 + 1] - tables[0][self.k0]))
        p = copy_params(self.params)
        p.x0_lon[0] = s0
        L = self.L - self.s0 + s0 if self.mode == LON_STOPPING else self.L
        return tables, (lambda flags: PlanInputs(_flagged(p, flags), self.cost, self.T, traj_len_of(self.T, DT), L, self.D))


def _flagged(p, flags):
    q = copy_params(p)
    q.flags = flags
    return q


def uniform(n, h=1.0):
    return np.full(n - 1, h)


def irregular(n, seed, short=0.05, share=0.1):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n - 1) < share, short, rng.uniform(0.5, 2.0, n - 1))


FULL_T = [3.0]                       # N dt with N = 30: no step is extrapolated
SHORT_T = [0.6, 0.8, 1.0]
MIXED_T = [0.8, 1.4, 2.0, 3.0]
SPEEDS = np.linspace(6.0, 12.0, 5)


def _scenes():
    s = {}
    # 1-3: all workgroups inside | all outside | both kinds in one launch
    s["all_inside"] = (lambda: Scene(uniform(144), 40, 9.0, FULL_T, SPEEDS), dict(win_n=64, inside=True, outside=False))
    s["all_outside"] = (lambda: Scene(uniform(144), 40, 9.0, SHORT_T, SPEEDS), dict(inside=False, outside=True))
    s["both_kinds"] = (lambda: Scene(uniform(160), 40, 9.0, MIXED_T, SPEEDS), dict(win_n=64, inside=True, outside=True))
    # 4: each window size, the whole block, the smallest reference that windows and the largest that does not
    s["size_16"] = (lambda: Scene(uniform(128), 50, 1.5, FULL_T, [1.0, 2.0], low=True), dict(win_n=16, inside=True))
    s["size_32"] = (lambda: Scene(uniform(128), 50, 5.0, FULL_T, [3.0, 5.0, 7.0]), dict(win_n=32, inside=True))
    s["size_64"] = (lambda: Scene(uniform(144), 60, 9.0, MIXED_T, [6.0, 12.0]), dict(win_n=64))
    s["size_128"] = (lambda: Scene(uniform(300), 100, 30.0, FULL_T, [28.0, 32.0, 36.0]), dict(win_n=128, inside=True))
    s["whole_block"] = (lambda: Scene(uniform(144), 30, 25.0, FULL_T, [24.0, 26.0]), dict(win_n=0))
    s["n96_windows"] = (lambda: Scene(uniform(96), 40, 1.5, MIXED_T, [1.0, 2.0], low=True), dict(win_n=16))
    s["n95_does_not"] = (lambda: Scene(uniform(95), 40, 1.5, MIXED_T, [1.0, 2.0], low=True), dict(win_n=0))
    # 5: the window at the start of the table; negative target velocities: valid steps with s < pos[0]
    s["at_start"] = (lambda: Scene(uniform(144), 1, 1.0, [2.0, 3.0], [-3.0, 0.0, 3.0, 5.0], frac=0.3, low=True), dict(k0=0, inside=True, outside=True, below_start=True))
    # 6: clamped at the end: slow pairs end short of the path's end and stay windowed, fast ones run past it (out of domain)
    s["at_end"] = (lambda: Scene(uniform(144), 130, 5.0, [2.0, 3.0], [1.0, 1.5, 2.0, 2.5, 6.0, 9.0], a0=0.0), dict(win_n=32, k0=144 - 32, inside=True, outside=True, beyond_end=True))
    # 7: a valid step in the last admissible segment w0 + wn - 5: constant speed, v0 the only sample, T = N dt: s(T) is the rule's hi;
    #    24 segments ahead + 8 = 32 vertices
    s["last_segment"] = (lambda: Scene(uniform(144), 50, 8.0, FULL_T, [8.0], a0=0.0), dict(win_n=32, inside=True, outside=False, last_segment=True))
    # 8: a valid step in the first admissible segment w0 + 2 (w0 == 0, the plan starts in segment 2)
    s["first_segment"] = (lambda: Scene(uniform(144), 2, 8.0, FULL_T, [6.0, 8.0, 10.0], a0=0.0, frac=0.25), dict(k0=0, inside=True, first_segment=True))
    # 9: irregular spacing with many short segments: hundreds of bucket entries per window
    s["short_segments"] = (lambda: Scene(irregular(200, 5), 60, 9.0, MIXED_T, SPEEDS), dict(min_buckets=257, inside=True, outside=True))
    s["short_segments_full_T"] = (lambda: Scene(irregular(220, 6), 90, 7.0, FULL_T, [5.0, 7.0, 9.0]), dict(min_buckets=257, inside=True))
    # 10: stopping mode and low-velocity mode (lat_T comes from s(T)), and both
    s["stopping"] = (lambda: Scene(uniform(160), 40, 6.0, MIXED_T, [6.0, 10.0, 14.0], stopping=True, a0=-0.3), dict(inside=True, outside=True))
    s["low_velocity"] = (lambda: Scene(uniform(160), 40, 1.5, MIXED_T, [0.5, 1.5, 3.0], low=True), dict(inside=True))
    s["stopping_low_velocity"] = (lambda: Scene(uniform(160), 40, 2.0, MIXED_T, [2.0, 4.0, 6.0], stopping=True, low=True, a0=-0.1), dict(inside=True))
    return s


SCENES = _scenes()


# ---- running and comparing -------------------------------------------------------------------------------------------------------
class Pair:
    """the module's two contexts: `ctx` (default options) and the poison context"""

    def __init__(self):
        self.ctx = RpContext(0)
        self.poison_ctx = RpContext(0)
        self.poison_ctx.set_option("table_window", 0)
        self.defaults = {k: self.ctx.get_option(k) for k in ("table_window", "lanes", "auto_materialize", "winner_skip_query")}
        self.scene = None

    def close(self):
        self.ctx.close()
        self.poison_ctx.close()

    def setup(self, scene):
        self.scene = scene
        self.ctx.set_coordinate_system(scene.co)
        self.ctx.set_obstacles(scene.obs)
        tables, self.poison_inputs = scene.poison()
        self.poison_ctx.set_reference(*tables)
        self.poison_ctx.set_obstacles(scene.obs)

    def poison(self, flags, lo=0, hi=-1, want=True, options=()):
        for k, v in options:
            self.poison_ctx.set_option(k, v)
        self.poison_ctx.plan(self.poison_inputs(flags), lo, hi, want_best_states=want)
        assert self.poison_ctx.get_option("last_table_window") == 0

    def check_window(self, windowed=True):
        """single launch, and the window the rule gives for the scene"""
        w = self.scene.window
        assert self.ctx.get_option("last_single_launch") == 1
        assert self.ctx.get_option("last_table_window") == (w.n if windowed else 0)
        assert self.ctx.get_option("last_table_window_first") == (w.k0 if windowed else 0)


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    for k, v in p.defaults.items():
        p.ctx.set_option(k, v)
    p.close()


_ORACLE = {}


def oracle_run(key, inp, scene, lo=0, hi=-1):
    """the oracle's plan, computed once per (scene, flags, range) and left unchanged"""
    from oracle import oracle
    if key not in _ORACLE:
        _ORACLE[key] = oracle.plan(inp, oracle.OracleTables.from_coordinate_system(scene.co, scene.obs), lo, hi)
    return _ORACLE[key]


def grab(ctx, out, rows):
    status, cost = ctx.fetch_status()
    return dict(out=out, status=status, cost=cost, states=ctx.fetch_states() if rows else None)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same_bits(a, b, what):
    found = status_cost_differences(a["status"], a["cost"], b["status"], b["cost"]) + output_differences(a["out"], b["out"])
    for f in ("n_candidates", "n_infeasible_kinematics"):
        if getattr(a["out"], f) != getattr(b["out"], f):
            found.append(f"{f}: {getattr(a['out'], f)} / {getattr(b['out'], f)}")
    sa, sb = a["out"].best_states, b["out"].best_states
    if (sa is None) != (sb is None) or (sa is not None and not np.array_equal(bits(sa), bits(sb))):
        found.append("the winner's state block differs")
    for f in ("best_lon_coeffs", "best_lat_coeffs"):
        if a["out"].best_index >= 0 and not np.array_equal(bits(getattr(a["out"], f)), bits(getattr(b["out"], f))):
            found.append(f"{f} differ")
    if a["states"] is not None:
        bad = np.flatnonzero((bits(a["states"]) != bits(b["states"])).reshape(len(a["status"]), -1).any(axis=1))
        if len(bad):
            found.append(f"state rows of {len(bad)} candidates differ, first {int(bad[0])}")
    assert not found, f"{what}: window / whole block: " + "; ".join(found)


def assert_oracle(run, orun, ctx, draw, lo=0):
    _compare_status(run["status"], run["cost"], orun, ctx, run["out"], lo)
    out, oout = run["out"], orun.out
    if out.best_states is not None or oout.best_index < 0:
        _compare_out(out, oout, ctx)
    else:   # a plan that was not asked for the winner's rows: everything but them
        assert out.best_index == oout.best_index and out.n_candidates == oout.n_candidates and out.n_feasible == oout.n_feasible
        _compare_collision_counts(out, oout, ctx)
        np.testing.assert_array_equal(out.reason_counts[1:7], oout.reason_counts[1:7])
        np.testing.assert_allclose(out.best_cost, oout.best_cost, rtol=COST_RTOL)
    if run["states"] is not None:
        lab = orun.status & 3
        defined = np.ones_like(lab, dtype=bool) if draw else ((lab == 1) | (lab == 3))
        np.testing.assert_allclose(run["states"][defined], orun.states[defined], rtol=0, atol=STATE_ATOL)


def three_ways(pair, scene, name, flags=0, want=True, rows=None, lo=0, hi=-1, options=()):
    """(c) poison, the windowed plan, (b) the same plan on the whole block, (a) the oracle.  Returns the windowed run and the lanes."""
    ctx = pair.ctx
    rows = bool(flags & FLAG_MATERIALIZE_ALL) if rows is None else rows
    inp = scene.inputs(flags)
    for k, v in options:
        ctx.set_option(k, v)
    try:
        pair.poison(flags, lo, hi, want, options)
        out = ctx.plan(inp, lo, hi, want_best_states=want)
        pair.check_window()
        lanes = ctx.get_option("last_lanes")
        win = grab(ctx, out, rows)
        ctx.set_option("table_window", 0)
        out0 = ctx.plan(inp, lo, hi, want_best_states=want)
        pair.check_window(windowed=False)
        assert ctx.get_option("last_lanes") == lanes
        whole = grab(ctx, out0, rows)
    finally:
        ctx.set_option("table_window", 1)
        for k, _ in options:
            ctx.set_option(k, pair.defaults[k])
            pair.poison_ctx.set_option(k, pair.defaults[k])
    assert_same_bits(win, whole, name)
    assert_oracle(win, oracle_run((name, flags, lo, hi), inp, scene, lo, hi), ctx, bool(flags & FLAG_DRAW_ALL), lo)
    return win, lanes


def check_classes(scene, lanes, want, name, cand_begin=0, n_cand=None):
    w = scene.window
    if "win_n" in want:
        assert w.n == want["win_n"], (name, w)
    if "k0" in want:
        assert w.k0 == want["k0"], (name, w)
    if "min_buckets" in want:
        assert w.n > 0 and w.nb >= want["min_buckets"], (name, w)
    if w.n == 0:
        return None
    cls, flags = scene.classes(lanes, cand_begin, n_cand)
    assert cls.margin >= MARGIN, (name, cls)
    if "inside" in want:
        assert (cls.inside > 0) == want["inside"], (name, cls)
    if "outside" in want:
        assert (cls.outside > 0) == want["outside"], (name, cls)

    S, valid = scene.valid_positions()
    seg = np.searchsorted(scene.pos, S, "right") - 1
    inside = (S >= w.s_lo) & (S < w.s_hi)
    if want.get("below_start"):
        assert w.s_lo == scene.pos[0] and (S[valid] < scene.pos[0]).any()
    if want.get("beyond_end"):
        assert w.s_hi == scene.pos[-1] and (S[valid] > scene.pos[-1]).any() and (S[valid].reshape(-1) < scene.pos[-1]).any()
    if want.get("last_segment"):
        assert (seg[valid & inside] == w.k0 + w.n - 5).any() and seg[valid].max() == w.k0 + w.n - 5
    if want.get("first_segment"):
        assert (seg[valid & inside] == w.k0 + 2).any()
    print(f"table window, scene {name}: window [{w.k0}, {w.k0 + w.n}) buckets {w.nb}, {lanes} lanes, workgroups inside {cls.inside} outside {cls.outside}, "
          f"margin {cls.margin:.3g} m")
    return cls


# ---- the tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_scene(pair, name):
    """scenes 1-10: production mode with the winner's rows (the plan keeps every row), and draw + materialize mode"""
    build, want = SCENES[name]
    scene = build()
    pair.setup(scene)
    win, lanes = three_ways(pair, scene, name)
    check_classes(scene, lanes, want, name)
    win2, lanes2 = three_ways(pair, scene, name, FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)
    if lanes2 != lanes:
        check_classes(scene, lanes2, want, name)
    if want.get("beyond_end"):   # the pairs that run past the end leave the projection domain there (reason 6); the oracle comparison holds every label
        S, valid = scene.valid_positions()
        past = np.repeat((np.where(valid, S, -np.inf) > scene.pos[-1]).any(axis=1), scene.nD)
        assert past.any() and not past.all()
        assert (((win["status"] >> 4) & 7)[past] == 6).any()


INSTANCE_HORIZONS = {31: 32, 50: 64, 70: 16}   # N + 1 -> lanes per candidate of the plans that keep rows


@pytest.mark.parametrize("obstacles,level", [("none", 0), ("dynamic", 1), ("static", 2)])
@pytest.mark.parametrize("n_steps", [16, 31, 50, 70])
def test_every_instance_with_the_prologue(pair, n_steps, obstacles, level):
    """Fused mode without rows (16 lanes at every horizon; N + 1 = 16: the one-step-block instance), materialize mode and draw +
    materialize mode (32 lanes up to 32 steps, 64 up to 64, 16 beyond -- there by option "lanes": by the rule such plans take two
    kernels), each without a collision query, against a dynamic-obstacle table and against static shapes as well."""
    N = n_steps - 1
    T = [0.8, 1.4, round(0.6 * N * DT, 1), N * DT] if N > 20 else [0.5, 0.8, N * DT]
    scene = Scene(uniform(280), 60, 9.0, T, [4.0, 7.0, 10.0], nD=8, N=N, obstacles=obstacles)
    pair.setup(scene)
    name = f"instance_n{n_steps}_{obstacles}"
    assert scene.window.n in (32, 64, 128)
    win, lanes = three_ways(pair, scene, name + "_fused", 0, want=False, rows=False)
    assert lanes == 16 and pair.ctx.get_option("last_collision_level") == level
    check_classes(scene, lanes, dict(inside=True, outside=True), name)
    if n_steps == 16:
        return
    want_lanes = INSTANCE_HORIZONS[n_steps]
    opts = (("lanes", 16),) if n_steps > 64 else ()
    for flags in (FLAG_MATERIALIZE_ALL, FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL):
        win, lanes = three_ways(pair, scene, name, flags, options=opts)
        assert lanes == want_lanes and pair.ctx.get_option("last_collision_level") == level
        check_classes(scene, lanes, dict(outside=True), name)


def test_eval_one_inherits_the_window(pair):
    """rp_eval_one after a windowed plan (draw + materialize mode: every candidate has rows): one candidate of a workgroup that missed,
    one of a workgroup that did not, the last one and the winner -- the batch's bits"""
    build, want = SCENES["both_kinds"]
    scene = build()
    pair.setup(scene)
    ctx = pair.ctx
    flags = FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL
    pair.poison(flags)
    out = ctx.plan(scene.inputs(flags))
    pair.check_window()
    lanes = ctx.get_option("last_lanes")
    run = grab(ctx, out, True)
    cls, missed_flags = scene.classes(lanes)
    gpb = W.RP_BLOCK // lanes
    missed, kept = missed_flags.index(True), missed_flags.index(False)
    for cand in (missed * gpb + 1, kept * gpb + 2, scene.n_candidates - 1, max(out.best_index, 0)):
        pair.poison(flags, cand, cand + 1)
        st, s1, c1 = ctx.eval_one(cand)
        assert np.array_equal(bits(st), bits(run["states"][cand])), cand
        assert s1 == run["status"][cand]
        assert (np.isnan(c1) and np.isnan(run["cost"][cand])) or bits([c1])[0] == bits([run["cost"][cand]])[0]


@pytest.mark.parametrize("skip_query", [1, 0])
def test_winner_reevaluation_inherits_the_window(pair, skip_query):
    """a production-mode plan that keeps no rows: the winner is evaluated again, by a launch that carries the plan's window"""
    scene = Scene(uniform(160), 40, 9.0, MIXED_T, SPEEDS, obstacles="dynamic")
    pair.setup(scene)
    opts = (("auto_materialize", 0), ("winner_skip_query", skip_query))
    win, lanes = three_ways(pair, scene, f"winner_reevaluation_{skip_query}", 0, rows=False, options=opts)
    assert win["out"].best_index >= 0 and win["out"].best_states is not None
    cls, flags = scene.classes(lanes)
    assert cls.inside > 0 and cls.outside > 0
    # ... and the rows are the ones of the plan that keeps them all
    full, _ = three_ways(pair, scene, "winner_reevaluation_rows", FLAG_MATERIALIZE_ALL)
    assert full["out"].best_index == win["out"].best_index
    np.testing.assert_allclose(win["out"].best_states, full["states"][full["out"].best_index], rtol=0, atol=1e-9)


def test_shards_inherit_the_window(pair):
    """two shards of a grid: the window comes from the whole grid's samples whatever the range; status and cost bits of both are the
    unsharded plan's"""
    build, want = SCENES["both_kinds"]
    scene = build()
    pair.setup(scene)
    full, lanes = three_ways(pair, scene, "shards_full", 0, want=False, rows=False)
    C = scene.n_candidates
    cut = C // 2 + 3
    for lo, hi in ((0, cut), (cut, C)):
        part, lanes_p = three_ways(pair, scene, "shards", 0, want=False, rows=False, lo=lo, hi=hi)
        assert lanes_p == lanes
        found = status_cost_differences(full["status"][lo:hi], full["cost"][lo:hi], part["status"], part["cost"])
        assert not found, f"shard [{lo}, {hi}): " + "; ".join(found)
        cls, flags = scene.classes(lanes, lo, hi - lo)
        assert cls.margin >= MARGIN
        print(f"table window, shard [{lo}, {hi}): workgroups inside {cls.inside} outside {cls.outside}")


def test_level_chain_inherits_the_window(pair):
    """three levels through plan_levels_begin: the first two have no winner (from 9 m/s to 36 m/s and more within 3 s is beyond a_max for
    every time sample) and a window of 128 vertices, the third is the plan of `both_kinds` with its window of 64; against the same
    chain on the whole block, and the third level against the oracle"""
    scene = Scene(uniform(280), 40, 9.0, MIXED_T, SPEEDS)
    pair.setup(scene)
    ctx = pair.ctx
    tl = traj_len_of(scene.T, DT)
    wild = np.array([36.0, 38.0])
    assert W.rule_window(scene.pos, scene.bk, scene.mode, scene.x0_lon, scene.T, wild).n == 128 and scene.window.n == 64
    levels = [(scene.T, tl, wild, scene.D[:3]), (scene.T, tl, wild, scene.D), (scene.T, tl, scene.L, scene.D)]
    runs = []
    try:
        for tw in (1, 0):
            ctx.set_option("table_window", tw)
            pair.poison(0)
            ctx.plan_levels_begin(scene.params, scene.cost, levels)
            out = ctx.plan_wait()
            assert ctx.last_level() == 2 and out.best_index >= 0
            pair.check_window(windowed=bool(tw))
            runs.append(grab(ctx, out, False))
    finally:
        ctx.set_option("table_window", 1)
    assert_same_bits(runs[0], runs[1], "level chain")
    assert_oracle(runs[0], oracle_run(("level_chain", 0, 0, -1), scene.inputs(), scene), ctx, False)


@pytest.mark.parametrize("seed", range(10))
def test_random_plans(pair, seed):
    """random polyline spacing, start, grids; production mode and draw + materialize mode"""
    rng = np.random.default_rng(900 + seed)
    n = int(rng.integers(100, 260))
    seg = irregular(n, 50 + seed, short=float(rng.uniform(0.15, 0.3)), share=float(rng.uniform(0.0, 0.15))) if seed % 2 else \
        rng.uniform(0.6, 1.8, n - 1)
    N = int(rng.choice([20, 30, 45, 60]))
    stopping, low = bool(seed % 3 == 2), bool(seed % 4 == 1)
    v0 = float(rng.uniform(1.0, 3.0) if low else rng.uniform(4.0, 14.0))
    nT = int(rng.integers(1, 5))
    T = np.unique(np.round(rng.uniform(0.6, N * DT, nT), 1))
    if seed % 2 == 0:
        T = np.unique(np.append(T, N * DT))
    k0 = int(rng.integers(0, n - 2))
    if stopping:
        L = np.sort(rng.uniform(0.3, 1.1, int(rng.integers(1, 5)))) * v0 * T.max()
    else:
        L = np.sort(rng.uniform(max(0.0, v0 - 4.0), v0 + 4.0, int(rng.integers(1, 6))))
    scene = Scene(seg, k0, v0, T, L, nD=int(rng.integers(3, 9)), N=N, a0=float(rng.uniform(-1.0, 1.0)), frac=float(rng.uniform(0.05, 0.95)),
                  low=low, stopping=stopping, obstacles=("none", "dynamic", "static")[seed % 3])
    pair.setup(scene)
    name = f"random_{seed}"
    for flags in (0, FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL):
        win, lanes = three_ways(pair, scene, name, flags)
        w = scene.window
        if w.n == 0:
            print(f"table window, {name}: n {n}, N {N}, {scene.n_candidates} candidates, {lanes} lanes: the whole block")
            continue
        cls, _ = scene.classes(lanes)
        assert cls.margin >= MARGIN, (name, cls)
        print(f"table window, {name}: n {n}, N {N}, {scene.n_candidates} candidates, {lanes} lanes, window [{w.k0}, {w.k0 + w.n}) buckets {w.nb}: "
              f"workgroups inside {cls.inside} outside {cls.outside}")
