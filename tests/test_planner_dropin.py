"""This build's planner against the REFERENCE's own behaviour, recorded in tests/golden/reference_runs/ by
tests/golden/make_reference_runs.py (which runs the unmodified reference under the third-party stand-ins of
tests/golden/_ref_shims.py): the candidate order of the reference's sampling on random configurations, and whole plan() cycles on
random cases.  The planner's backend here is the oracle-backed context (CPU).
"""
import os

import numpy as np

from _golden import REFERENCE_RUNS_DIR, random_plan_cases, random_sampling_trials
from _oracle_ctx import OracleContext


def test_candidate_order_matches_reference_sampling_on_random_configurations():
    """``FixedIntervalSampling.grids_at_level`` / ``grid_sets_at_level`` (the batch views the device path is fed from) against the
    REFERENCE's ``generate_trajectories_at_level`` (sampling.py:202-242) on random sampling configurations: the (T, lon, d) sequence of
    the reference's candidate list must be the product order of the grids -- including vehicles that sit exactly on a lateral sample
    (the union is then a copy of the set, whose iteration order may differ from the set's own), stopping mode with goals behind the
    vehicle, and both velocity regimes.  The reference's candidate lists: tests/golden/reference_runs/sampling_order.npz."""
    from commonroad_rp_amd import _capi
    orders = np.load(os.path.join(REFERENCE_RUNS_DIR, "sampling_order.npz"))
    checked = on_sample = 0
    for tr in random_sampling_trials():
        trial, ours, level, x0_lon, x0_lat, pick = tr.trial, tr.ours, tr.level, tr.x0_lon, tr.x0_lat, tr.pick
        on_sample += pick
        mode = tr.cfg.sampling.longitudinal_mode
        got = orders[f"t{trial}"]   # (stopping: the list as _get_optimal_trajectory filters it first, reactive_planner.py:1076-1077)
        T, tl, L, D = ours.grids_at_level(level, x0_lon, x0_lat, mode)
        want = np.array([[t, l, d] for t in T for l in L for d in D], dtype=float).reshape(-1, 3)
        # (velocity keeping: a quartic's end condition is x_d = [v, 0]; stopping: a quintic's [s, 0, 0] -- the first entry either way;
        #  a longitudinal polynomial without coefficients drops its lateral loop in the reference: none here, all solvable)
        assert got.shape == want.shape, (trial, got.shape, want.shape)
        np.testing.assert_array_equal(got, want, err_msg=f"trial {trial}: level {level}, mode {mode}, d0 on a sample: {pick}")
        # the set view the extension module iterates itself: same sequences
        g4 = ours.grid_sets_at_level(level, x0_lon, mode)
        Ls = np.fromiter(g4[2], np.float64, len(g4[2])) if isinstance(g4[2], (set, frozenset)) else g4[2]
        u = g4[3].union((x0_lat[0],))
        np.testing.assert_array_equal(Ls, L)
        np.testing.assert_array_equal(np.fromiter(u, np.float64, len(u)), D)
        np.testing.assert_array_equal(g4[0], T)
        # ... and rp_plan_cycle's emulation of the lateral set in C (the insertion sequence is the level's linspace)
        lv = ours.cycle_level(level, mode)
        if lv is not None and x0_lat[0] == 0.0:
            np.testing.assert_array_equal(_capi.pyset_order(lv[3], True), D)
        checked += len(want)
    assert checked > 5000 and on_sample >= 30


def test_own_planner_matches_live_reference_plan_on_random_cases():
    """This build's ``ReactivePlanner`` (oracle-backed context: host logic + restated arithmetic) against the reference's ``plan()`` on
    further draws of make_golden.random_cases (its runs: tests/golden/reference_runs/random_plan_*.npz, make_reference_runs.py) -- whole
    cycles: level loop, counters, output packing -- a third of them with the vehicle exactly on a lateral sample of the level
    (candidate order = iteration order of a COPY of the sample set)."""
    from _golden import build_planner_from_plan_golden, compare_plan_result
    done = planned = 0
    for name in random_plan_cases(n=30, seed0=7000):
        out = dict(np.load(os.path.join(REFERENCE_RUNS_DIR, name + ".npz")))
        rp, z = build_planner_from_plan_golden(out, OracleContext)
        res = rp.plan()
        compare_plan_result(res, rp, z, atol=1e-9)
        done += 1
        planned += res is not None
    assert done == 30 and planned >= 10
