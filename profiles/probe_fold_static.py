"""What the static-shape machinery of the COLL = 2 evaluation kernel costs next to a dynamic table, and what checking a few static
rectangles as rows of the dynamic table ("fold_static") gives back.  Draw mode (every candidate evaluated, rows stored), cfg3's grid.

  ceiling   cfg3f as it is (no static shape: COLL = 1) against cfg3f plus ONE rectangle 1 km from the route (COLL = 2, the same
            collision results): the difference is what the grid lookup, the static masks and the cluster walk cost when they find nothing.
  fold      (library with the option "fold_static") cfg3 with fold_static = 0 against = 1, and cfg3f plus k = 1, 2, 4, 8 rectangles
            9 m beside the route with both settings: the sweep behind the threshold on n_sobb.

Variants alternate within one process, `rounds` times behind one unrecorded round; per variant and round: median kernel_ms of 30 profiled plans (HIP events on the
launch) and the wall time per step of 200 plans bracketed by the call's own synchronisation.
usage (GPU box): python profiles/probe_fold_static.py <ceiling|fold> [rounds]"""
import os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd")]
from commonroad_rp_amd import workloads as W, _capi
from commonroad_rp_amd._capi import RpContext, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL, PlanInputs, copy_params
from commonroad_rp_amd.collision import ObstacleTables

what = sys.argv[1] if len(sys.argv) > 1 else "ceiling"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
print("library", _capi.source_hash(), "probe", what, "rounds", rounds, flush=True)


def with_rectangles(w, rects):
    ob = w.obstacles
    return ObstacleTables(static_obb=np.asarray(rects, dtype=float).reshape(-1, 5), dyn_obb=ob.dyn_obb, dyn_t0=ob.dyn_t0)


def beside_route(w, k, offset=-9.0):
    """k parked-vehicle rectangles (2.25 x 1.0 m half extents) along the route, `offset` m to the side that has no traffic."""
    co = w.coordinate_system
    s0 = w.inputs.params.x0_lon[0]
    out = []
    for j in range(k):
        s = s0 + 10.0 + 12.0 * j
        p = co.convert_to_cartesian_coords(s, offset)
        kk = min(int(np.searchsorted(co.ref_pos, s, side="right")) - 1, len(co.ref_pos) - 2)
        out.append((p[0], p[1], co.ref_theta[kk], 2.25, 1.0))
    return out


class Variant:
    def __init__(self, label, w, tables=None, fold=None):
        self.label, self.ctx = label, RpContext(0)
        self.ctx.set_coordinate_system(w.coordinate_system)
        self.ctx.set_obstacles(tables if tables is not None else w.obstacles)
        if fold is not None:
            self.ctx.set_option("fold_static", fold)
        p = copy_params(w.inputs.params)
        p.flags |= FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL
        self.inp = PlanInputs(p, w.inputs.cost, w.inputs.T, w.inputs.traj_len, w.inputs.L, w.inputs.D)
        for _ in range(8):
            self.out = self.ctx.plan(self.inp)
        self.kernel, self.step = [], []

    def round(self):
        c = self.ctx
        c.set_profiling(1)
        self.kernel.append(float(np.median([c.plan(self.inp).kernel_ms for _ in range(30)])))
        c.set_profiling(0)
        for _ in range(10):
            c.plan(self.inp)
        t0 = time.perf_counter()
        for _ in range(200):
            c.plan(self.inp)
        self.step.append((time.perf_counter() - t0) / 200 * 1e3)

    def level(self):
        try:
            return self.ctx.get_option("last_collision_level")
        except Exception:
            return -1

    def report(self):
        o, k, s = self.out, np.array(self.kernel) * 1e3, np.array(self.step) * 1e3
        print(f"{self.label:22s} level {self.level():2d} best {o.best_index:6d} free {o.n_feasible - o.n_collision:6d}  kernel us "
              f"median {np.median(k):7.2f} min {k.min():7.2f} max {k.max():7.2f}   step us median {np.median(s):7.2f} min {s.min():7.2f} "
              f"max {s.max():7.2f}   rounds(kernel) {' '.join(f'{v:.2f}' for v in k)}", flush=True)


def run(variants):
    for r in range(rounds + 1):   # round 0 is not recorded: the clocks settle in it (the first variant's first round read 6 % high)
        for v in variants:
            v.round()
            if r == 0:
                v.kernel.clear(); v.step.clear()
    for v in variants:
        v.report()
        v.ctx.close()


if what == "ceiling":
    w = W.cfg3f()
    co = w.coordinate_system
    far = co.convert_to_cartesian_coords(w.inputs.params.x0_lon[0], 0.0)
    run([Variant("cfg3f", w), Variant("cfg3f+1 rect at 1 km", w, with_rectangles(w, [(far[0] + 1000.0, far[1] + 1000.0, 0.0, 2.25, 1.0)]))])
else:
    w3, wf = W.cfg3(), W.cfg3f()
    vs = [Variant("cfg3 fold 0", w3, fold=0), Variant("cfg3 fold 1", w3, fold=1), Variant("cfg3f", wf)]
    for k in (1, 2, 4, 8):
        t = with_rectangles(wf, beside_route(wf, k))
        vs += [Variant(f"cfg3f+{k} fold 0", wf, t, fold=0), Variant(f"cfg3f+{k} fold 1", wf, t, fold=1)]
    run(vs)
