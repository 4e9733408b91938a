"""Loader for the golden fixtures in tests/golden/*.npz (see tests/golden/make_golden.py)."""
from __future__ import annotations

import glob
import os

import numpy as np

from commonroad_rp_amd._capi import PlanInputs, make_params, make_cost, FLAG_DRAW_ALL
from commonroad_rp_amd.collision import ObstacleTables

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case_names():
    # (cfg<k>_ref*: BASELINE.json's configurations at full size, tests/test_baseline_reference.py)
    import re
    return sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
                  if not n.startswith(("scenario_", "plan_", "frontend_", "corridor_", "loop_")) and not re.match(r"cfg\d_ref", n))


class Golden:
    def __init__(self, name: str):
        self.name = name
        self.z = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
        z = self.z
        veh = z["vehicle"]
        flags = FLAG_DRAW_ALL if int(z["draw"]) else 0
        params = make_params(dt=float(z["dt"]), N=int(z["N"]), factor=int(z["factor"]), time_step0=int(z["time_step0"]),
                             low_vel_mode=bool(z["low_vel_mode"]), lon_mode=int(z["lon_mode"]),
                             constraint_mask=int(z["constraint_mask"]), flags=flags, x0_lon=z["x0_lon"],
                             x0_lat=z["x0_lat"], x0_orientation=float(z["x0_orientation"]), wheelbase=veh[0],
                             wb_rear_axle=veh[1], length=veh[2], width=veh[3], a_max=veh[4], v_switch=veh[5],
                             delta_max=veh[6], v_delta_max=veh[7])
        ds, dss = float(z["desired_speed"]), float(z["desired_s"])
        cost = make_cost(kind=int(z["cost_kind"]), w_a=float(z["w_a"]), desired_speed=None if np.isnan(ds) else ds,
                         desired_d=float(z["desired_d"]), desired_s=None if np.isnan(dss) else dss)
        self.inputs = PlanInputs(params, cost, z["T"], z["traj_len"], z["L"], z["D"])
        self.obstacles = ObstacleTables(static_obb=z["static_obb"], static_tri=z["static_tri"],
                                        static_circ=z["static_circ"], dyn_obb=z["dyn_obb"], dyn_t0=int(z["dyn_t0"]))
        self.draw = bool(int(z["draw"]))

    def __getitem__(self, k):
        return self.z[k]

    def oracle_tables(self):
        from oracle.oracle import OracleTables
        z = self.z
        return OracleTables(z["ref_pos"], z["ref_theta"], z["ref_curv"], z["ref_curv_d"], z["ref_path"],
                            float(z["proj_d_limit"]), self.obstacles)

    def setup_context(self, ctx):
        z = self.z
        ctx.set_reference(z["ref_pos"], z["ref_theta"], z["ref_curv"], z["ref_curv_d"], z["ref_path"],
                          float(z["proj_d_limit"]))
        ctx.set_obstacles(self.obstacles)


def scenario_from_tables(tb: ObstacleTables, road_boundary_triangles=None):
    """A duck-typed CommonRoad scenario (``static_obstacles`` / ``dynamic_obstacles`` with ``obstacle_shape``,
    ``initial_state``, ``prediction.trajectory.state_list``) holding the content of obstacle tables: what
    ``set_collision_checker(scenario=...)`` reads (reference: commonroad_rp/reactive_planner.py:233-251).  Dynamic
    rows must be present over one contiguous range of steps, with constant extents."""
    from types import SimpleNamespace as NS
    static = []
    for r in tb.static_obb:
        static.append(NS(obstacle_shape=NS(length=2.0 * r[3], width=2.0 * r[4]), prediction=None,
                         initial_state=NS(time_step=0, position=np.array(r[0:2]), orientation=float(r[2]))))
    for r in tb.static_circ:
        static.append(NS(obstacle_shape=NS(radius=float(r[2])), prediction=None,
                         initial_state=NS(time_step=0, position=np.array(r[0:2]), orientation=0.0)))
    dynamic = []
    for row in tb.dyn_obb:
        present = np.flatnonzero(~np.isnan(row[:, 0]))
        if len(present) == 0:
            continue
        assert np.array_equal(present, np.arange(present[0], present[-1] + 1)), "contiguous steps expected"
        states = [NS(time_step=int(tb.dyn_t0 + k), position=np.array(row[k, 0:2]), orientation=float(row[k, 2])) for k in present]
        dynamic.append(NS(obstacle_shape=NS(length=2.0 * row[present[0], 3], width=2.0 * row[present[0], 4]),
                          initial_state=states[0],
                          prediction=NS(trajectory=NS(state_list=states[1:])) if len(states) > 1 else NS(trajectory=NS(state_list=[]))))
    tri = tb.static_tri if road_boundary_triangles is None else road_boundary_triangles
    return NS(static_obstacles=static, dynamic_obstacles=dynamic, lanelet_network=None,
              road_boundary_triangles=np.asarray(tri, dtype=float).reshape(-1, 6))


def plan_case_names():
    return sorted(n for n in (os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "plan_*.npz"))))


def build_planner_from_plan_golden(name, backend_factory, planner_cls=None, overrides=None):
    """Set up a planner exactly as tests/golden/make_golden.py::make_planner did for the reference.  ``overrides``: entries that
    replace / complete the fixture's (the loop fixtures carry no ``continuous`` / ``via_scenario`` / ``planned``).  ``name``: a fixture's
    name, or the dictionary a fixture would hold (a reference run made by the test itself)."""
    from commonroad_rp_amd.config import ReactivePlannerConfiguration
    from commonroad_rp_amd.coordinate_system import CoordinateSystem
    from commonroad_rp_amd.reactive_planner import ReactivePlanner
    from commonroad_rp_amd.state import ReactivePlannerState
    z = dict(name) if isinstance(name, dict) else dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    z.update(overrides or {})
    cfg = ReactivePlannerConfiguration.from_dict(dict(
        planning=dict(dt=float(z["dt"]), time_steps_computation=int(z["N"]), factor=int(z["factor"]),
                      low_vel_mode_threshold=float(z["low_vel_mode_threshold"]),
                      continuous_collision_check=bool(int(z["continuous"]))),
        sampling=dict(longitudinal_mode="stopping" if int(z["lon_mode"]) else "velocity_keeping", t_min=float(z["t_min"])),
        debug=dict(draw_traj_set=bool(int(z.get("draw", 0))), show_plots=bool(int(z.get("draw", 0))))))
    cls = planner_cls or ReactivePlanner
    rp = cls(cfg, backend_factory=backend_factory)
    rp.set_reference_path(coordinate_system=CoordinateSystem(z["ref_path"], float(z["proj_d_limit"])))
    tables = ObstacleTables(static_obb=z["static_obb"], static_tri=z["static_tri"], static_circ=z["static_circ"],
                            dyn_obb=z["dyn_obb"], dyn_t0=int(z["dyn_t0"]))
    if int(z.get("via_scenario", 0)):
        # the reference built its checker from a scenario (reactive_planner.py:233-251): same entry here, so that
        # planning.continuous_collision_check reaches the obstacle side as well (:238-245)
        sc = scenario_from_tables(tables)
        rp.set_collision_checker(scenario=sc, road_boundary_obstacle=sc.road_boundary_triangles)
    else:
        rp.set_collision_checker(collision_checker=tables)
    x0 = ReactivePlannerState(time_step=int(z["time_step0"]), position=z["x0_position"], orientation=float(z["x0_orientation"]),
                              velocity=float(z["x0_velocity"]), steering_angle=0.0, acceleration=0.0, yaw_rate=0.0)
    rp.reset(initial_state_cart=x0, initial_state_curv=(list(z["x0_lon"]), list(z["x0_lat"])),
             collision_checker=rp.collision_checker, coordinate_system=rp.coordinate_system)
    if int(z["lon_mode"]):
        rp.set_desired_lon_position(float(z["desired_s"]), float(z["delta_s"][0]), float(z["delta_s"][1]))
    else:
        rp.set_desired_velocity(desired_velocity=float(z["desired_speed"]), current_speed=float(z["x0_velocity"]))
    if not np.isnan(z["v_range"][0]):
        rp.set_v_sampling_parameters(float(z["v_range"][0]), float(z["v_range"][1]))
    return rp, z


def compare_plan_result(res, rp, z, atol):
    assert (res is not None) == bool(int(z["planned"]))
    assert rp.infeasible_count_kinematics == int(z["n_infeasible_kinematics"])
    assert rp.infeasible_count_collision == int(z["n_infeasible_collision"])
    from commonroad_rp_amd._capi import REASON_NAMES
    got = [rp.infeasible_reason_dict.get(k, 0) for k in REASON_NAMES[1:6]]
    np.testing.assert_array_equal(got, z["reason_counts"])
    if res is None:
        return
    cart, cvln, lon_list, lat_list = res
    c = np.array([[st.time_step, st.position[0], st.position[1], st.orientation, st.velocity, st.acceleration, st.yaw_rate,
                   st.steering_angle] for st in cart.state_list], dtype=float)
    np.testing.assert_allclose(c, z["cart"], rtol=0, atol=atol)
    v = np.array([[st.time_step, st.position[0], st.position[1], st.orientation, st.velocity, st.acceleration, st.yaw_rate]
                  for st in cvln.state_list], dtype=float)
    np.testing.assert_allclose(v, z["cvln"], rtol=0, atol=atol)
    np.testing.assert_allclose(np.array(lon_list, dtype=float), z["lon_list"], rtol=0, atol=atol)
    np.testing.assert_allclose(np.array(lat_list, dtype=float), z["lat_list"], rtol=0, atol=atol)


LOOP_REASONS = ("velocity", "acceleration", "kappa", "kappa_dot", "yaw_rate")


def record_plan_stats(planner):
    """Wraps ``planner.plan`` (instance attribute; the reference's class or this build's) so that every call leaves a row
    [planned, low-velocity mode, infeasible_count_kinematics, infeasible_count_collision, the five reason counters, number of stored
    trajectories] in the returned list -- read right behind ``plan()``: the driver loop's ``reset()`` clears the counters
    (reactive_planner.py:186), so a callback behind it sees zeros."""
    rows = []
    inner = planner.plan

    def plan(*a, **k):
        res = inner(*a, **k)
        rd = planner._infeasible_reason_dict
        rows.append([int(res is not None), int(planner._low_vel_mode), int(planner._infeasible_count_kinematics),
                     int(planner._infeasible_count_collision)] + [int(rd.get(q, 0)) for q in LOOP_REASONS] +
                    [len(planner.stored_trajectories or [])])
        return res
    planner.plan = plan
    return rows


def random_sampling_trials(n: int = 120, seed: int = 11):
    """Random sampling configurations, initial states and levels (the draws of
    tests/test_planner_dropin.py::test_candidate_order_matches_reference_sampling_on_random_configurations; the reference's candidate
    order on them: tests/golden/reference_runs/sampling_order.npz, written by tests/golden/make_reference_runs.py).  Yields per trial
    a namespace with trial, cfg, ours (this build's FixedIntervalSampling on cfg), level, low_vel, stopping, x0_lon, x0_lat and pick
    (x0_lat[0] is a lateral sample of the level)."""
    from types import SimpleNamespace as NS
    from commonroad_rp_amd.sampling import FixedIntervalSampling
    rng = np.random.default_rng(seed)
    for trial in range(n):
        dt = float(rng.choice([0.1, 0.2]))
        N = int(rng.integers(10, 41))
        stopping = trial % 4 == 3
        levels = int(rng.integers(2, 5))
        d_min, d_max = -float(rng.choice([1.0, 1.5, 2.0, 3.0])), float(rng.choice([1.0, 2.0, 2.5, 3.0]))
        t_min = float(dt * int(rng.integers(2, max(3, N // 3))))
        cfg = NS(planning=NS(dt=dt, time_steps_computation=N),
                 sampling=NS(sampling_method=1, longitudinal_mode="stopping" if stopping else "velocity_keeping", num_sampling_levels=levels,
                             t_min=t_min, v_min=float(rng.uniform(0, 4)), v_max=float(rng.uniform(6, 20)), s_min=-float(rng.uniform(1, 8)),
                             s_max=float(rng.uniform(1, 8)), d_min=d_min, d_max=d_max))
        ours = FixedIntervalSampling(cfg)
        level = int(rng.integers(0, levels))
        low_vel = bool(trial % 5 == 0)
        x0_lon = [float(rng.uniform(0, 3)), float(rng.uniform(0.5, 3.0) if low_vel else rng.uniform(5, 15)), float(rng.normal(0, 0.3))]
        d_samples = sorted(ours.samples_d.samples_at_level(level))
        pick = trial % 3 == 0
        x0_lat = [float(d_samples[int(rng.integers(0, len(d_samples)))]) if pick else float(rng.uniform(d_min, d_max)), float(rng.normal(0, 0.1)), 0.0]
        yield NS(trial=trial, cfg=cfg, ours=ours, level=level, low_vel=low_vel, stopping=stopping, x0_lon=x0_lon, x0_lat=x0_lat, pick=pick)


def random_plan_cases(n: int = 30, seed0: int = 7000):
    """Names of the reference's plan() runs on draws of make_golden.random_cases (tests/golden/reference_runs/random_plan_<seed>_<k>.npz,
    written by tests/golden/make_reference_runs.py)"""
    return [f"random_plan_{seed0}_{k:02d}" for k in range(n)]


REFERENCE_RUNS_DIR = os.path.join(GOLDEN_DIR, "reference_runs")
