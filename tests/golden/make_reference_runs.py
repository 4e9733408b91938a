#!/usr/bin/env python3
"""Records of the reference planner's own runs that tests compare with, so that those tests need no copy of the reference
(``tests/golden/reference_runs/``, data only).  Runs the reference unmodified under the third-party stand-ins of ``_ref_shims.py``,
as make_golden.py does, and only where the reference is available:

    python tests/golden/make_reference_runs.py

  closed_loop.npz         the reference planner in the closed loop of tests/test_closed_loop.py (12 steps), state trace per case
  sampling_order.npz      the reference's candidate list as (T, lon end condition, d) per trial of _golden.random_sampling_trials
  random_plan_<seed>_<k>.npz  make_golden.run_plan_case on the draws of tests/test_planner_dropin.py's random plan() comparison
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "commonroad-reactive-planner_amd"))

import make_golden as mg  # noqa: E402  (installs the stand-ins and imports the reference)

from _golden import REFERENCE_RUNS_DIR, random_plan_cases, random_sampling_trials  # noqa: E402


def closed_loop_traces():
    from commonroad_rp_amd.harness import run_closed_loop
    from test_closed_loop import _trace
    out = {}
    cases = {c["name"]: c for c in mg.plan_cases()}
    for name in ("plan_arc_hv_obs", "plan_scurve_lv"):
        z = np.load(os.path.join(HERE, name + ".npz"))
        ref = mg.make_planner(dict(cases[name]))
        ref.record_state_and_input = lambda state, ref=ref: ref._record_state_list.append(state)   # InputState is a stand-in here
        res = run_closed_loop(ref, max_steps=12, desired_velocity=float(z["desired_speed"]))
        assert res.completed
        out[name] = _trace(res.states)
    return out


def sampling_order():
    from commonroad_rp.sampling import FixedIntervalSampling as RefSampling
    out = {}
    for t in random_sampling_trials():
        cand = RefSampling(t.cfg).generate_trajectories_at_level(t.level, t.x0_lon, t.x0_lat, t.cfg.sampling.longitudinal_mode, t.low_vel)
        if t.stopping:   # what _get_optimal_trajectory does to the list first (reactive_planner.py:1076-1077, trajectories.py:545-550)
            cand = [c for c in cand if c.trajectory_long.x_d[0] > t.x0_lon[0]]
        out[f"t{t.trial}"] = np.array([[c.trajectory_long.delta_tau, c.trajectory_long.x_d[0], c.trajectory_lat.x_d[0]] for c in cand],
                                      dtype=float).reshape(-1, 3)
    return out


def random_plans(n=30, seed0=7000):
    names = random_plan_cases(n, seed0)
    for k, case in enumerate(mg.random_cases(n=n, seed0=seed0)):
        case = dict(case, draw=False, cost_kind=0)
        case.pop("constraints", None)
        case.pop("level", None)
        if k % 3 == 0:   # on a sample of the first level plan() visits (level 1: 5 samples of [-3, 3]; three of them also at level 2 / 3)
            case["x0_lat"] = [float(np.linspace(-3, 3, 5)[1 + k % 3 + (k // 3) % 2]), case["x0_lat"][1], case["x0_lat"][2]]
        yield names[k], mg.run_plan_case(dict(case))


def main():
    os.makedirs(REFERENCE_RUNS_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(REFERENCE_RUNS_DIR, "closed_loop.npz"), **closed_loop_traces())
    np.savez_compressed(os.path.join(REFERENCE_RUNS_DIR, "sampling_order.npz"), **sampling_order())
    for name, out in random_plans():
        np.savez_compressed(os.path.join(REFERENCE_RUNS_DIR, name + ".npz"), **out)
    print("written:", sorted(os.listdir(REFERENCE_RUNS_DIR)))


if __name__ == "__main__":
    main()
