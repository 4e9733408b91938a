"""librp_pick.so exports what include/rp_pick.h declares and what the binding of commonroad_rp_amd.pick binds -- no more, no less; the
header stands on its own; without the library or without a GPU a TrajectoryPicker fails loudly.  Then, on the CPU alone, the yardstick
of tests/_pick.py: pinned to the reference planner's own decision on a draw fixture fed whole, and the conditions the GPU tests of
tests/test_pick.py rest on -- no first hit of a case hangs on 2e-6 m of the vehicle's size, no choice of a winner on 1e-9 of a cost, no
kinematic verdict on 1e-6 of a bound, and every case holds what its name says.  No compute calls on the device here."""
import ctypes as C
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, clearance, ensemble_check, lift, pick, trajectory_check, trajectory_score

import _lift as L
import _pick as P
import _score as S

SIBLINGS = (_capi, trajectory_check, ensemble_check, clearance, trajectory_score, lift)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(P.HEADER).read(), flags=re.S)


def _library():
    if not all(os.path.exists(m.LIB_PATH) for m in SIBLINGS + (pick,)):
        import __graft_entry__
        __graft_entry__.build()
    return pick.LIB_PATH


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    declared = sorted(set(re.findall(r"\b(rp_[a-z_]+)\s*\(", _header())))
    assert declared == sorted(pick.EXPORTED_SYMBOLS)
    assert len(declared) == 7 and all(name.startswith("rp_pick_") for name in declared)
    assert _exported(_library()) == declared
    # the other six libraries are what they were: nothing of the pick went into them, and nothing of theirs is exported here
    for m in SIBLINGS:
        assert not any(name.startswith("rp_pick") for name in m.EXPORTED_SYMBOLS)
        assert not set(m.EXPORTED_SYMBOLS) & set(declared)
        assert not any(name.startswith("rp_pick") for name in _exported(m.LIB_PATH)), m.LIB_PATH


def test_abi_version_struct_sizes_limits_and_package_exports(tmp_path):
    lib = pick.load_library(_library())
    assert lib.rp_pick_abi_version() == pick.ABI_VERSION == 1
    assert commonroad_rp_amd.TrajectoryPicker is pick.TrajectoryPicker
    assert commonroad_rp_amd.TrajectoryPickResult is pick.TrajectoryPickResult
    src = _header()
    assert int(re.search(r"#define\s+RP_PICK_ABI_VERSION\s+(\d+)", src).group(1)) == 1
    assert int(re.search(r"#define\s+RP_PICK_MAX_POSES\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", src).group(1)) == 24
    assert pick.MAX_POSES == lift.MAX_POSES == trajectory_check.MAX_POSES == 1 << 24
    assert (pick.TRAJ_POSES, pick.TRAJ_SWEPT) == (trajectory_check.TRAJ_POSES, trajectory_check.TRAJ_SWEPT) == (P.POSES, P.SWEPT)
    # the struct of the binding is the struct of the header, field by field, as the C compiler lays it out
    names = [n for n, _ in pick.RpPickResult._fields_]
    assert names == ["struct_size", "reserved_", "best", "best_cost", "n_feasible", "n_collision", "n_collision_before_best", "reason_counts"]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rp_pick.h"\nint main(void) {\n  rp_pick_result r = RP_PICK_RESULT_INIT;\n'
                    '  printf("%u %zu", r.struct_size, sizeof(rp_pick_result));\n' +
                    "".join(f'  printf(" %zu", offsetof(rp_pick_result, {n}));\n' for n in names) +
                    '  printf(" %zu %zu\\n", sizeof(rp_params), sizeof(rp_cost));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(P.REPO, "include"), "-o", str(exe), str(prog)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = C.sizeof(pick.RpPickResult)
    assert got == [want, want] + [getattr(pick.RpPickResult, n).offset for n in names] + [C.sizeof(_capi.RpParams), C.sizeof(_capi.RpCost)]
    assert want == 4 + 4 + 8 * 5 + 8 * 8 and pick.RpPickResult().struct_size == want
    assert [f.name for f in dataclasses.fields(pick.TrajectoryPickResult)] == [
        "status", "cost", "best", "best_cost", "best_states", "n_feasible", "n_collision", "n_collision_before_best", "reason_counts", "x", "y", "theta",
        "v", "a", "kappa", "kappa_dot", "theta_cl", "first_pose_hit", "first_segment_hit"]
    for name in ("set_reference", "set_obstacles", "pick", "close", "__enter__", "__exit__"):
        assert callable(getattr(pick.TrajectoryPicker, name))
    for name in ("label", "reason", "step"):
        assert isinstance(getattr(pick.TrajectoryPickResult, name), property)


def test_header_compiles_on_its_own(tmp_path):
    body = ("int uses(rp_pick *c, const rp_params *p, const rp_cost *k, rp_pick_result *r) {\n"
            "  return rp_pick_select(c, p, k, RP_TRAJ_POSES | RP_TRAJ_SWEPT, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, r, 0)\n"
            "         + rp_pick_set_reference(c, 0, 0, 0, 0, 0, 0, 20.0) + rp_pick_set_obstacles(c, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)\n"
            "         + (RP_PICK_MAX_POSES >= ((int64_t)1 << 24) ? 0 : 1) + RP_EINVAL + RP_PICK_ABI_VERSION + RP_N_ARRAYS; }\n")
    others = '#include "rp_check.h"\n#include "rp_ensemble.h"\n#include "rp_clearance.h"\n#include "rp_score.h"\n#include "rp_lift.h"\n'
    for name, includes in (("only_rp_pick", '#include "rp_pick.h"   /* first and only: the header must be self-contained */\n'),
                           ("pick_then_others", '#include "rp_pick.h"\n' + others), ("others_then_pick", others + '#include "rp_pick.h"\n')):
        src = tmp_path / f"{name}.c"
        src.write_text(includes + body)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(P.REPO, "include"), "-o", str(tmp_path / f"{name}.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        pick.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        pick.TrajectoryPicker(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        pick.TrajectoryPicker(0)


def test_makefile_targets_source_hash_inputs_and_capacities():
    src = open(P.SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "asm" not in re.sub(r"//.*", "", src)
    mk = open(os.path.join(P.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1)
    assert "pick" not in srcs and "rules" not in srcs
    assert re.search(r"^all:.*\$\(PICKLIB\)", mk, flags=re.M) and re.search(r"^pick-resource-usage:", mk, flags=re.M)
    assert re.search(r"^\$\(PICKLIB\): ", mk, flags=re.M) and re.search(r"^clean:\n\trm -f .*\$\(PICKLIB\)", mk, flags=re.M)
    # the libraries that include the shared rules are rebuilt when these change
    assert re.search(r"^\$\(CHECKLIB\):.* rp_check_rules\.h", mk, flags=re.M) and re.search(r"^PICKDEPS\s*:=.* rp_check_rules\.h", mk, flags=re.M)
    assert re.search(r"^\$\(LIFTLIB\): rp_lift_rules\.h rp_lift_walk\.inc$", mk, flags=re.M)
    assert re.search(r"^PICKDEPS\s*:=.* rp_lift_rules\.h rp_lift_walk\.inc ", mk, flags=re.M)
    # the files behind rp_source_hash() and the sibling libraries' own sources define nothing of the pick
    for name in srcs.split() + ["rp_check.hip", "rp_ensemble.hip", "rp_clearance.hip", "rp_score.hip", "rp_lift.hip", "rp_check_rules.h", "rp_lift_rules.h",
                               "rp_lift_walk.inc", "rp_session.h", "rp_obstacle_tables.h", "../commonroad_rp_amd/_session.py"]:
        text = open(os.path.join(P.CSRC, name)).read()
        assert "rp_pick_" not in text and "PK_" not in text, name
    # the capacities at which the pick switches to its device-memory variants are the siblings'
    assert P.LF_LDS_ROWS == L.LDS_ROWS == int(re.search(r"LF_LDS_ROWS\s*=\s*(\d+)", open(L.SOURCE).read()).group(1))
    assert P.CK_LDS_ROWS == int(re.search(r"CK_LDS_ROWS\s*=\s*(\d+)", open(os.path.join(P.CSRC, "rp_check.hip")).read()).group(1))
    # the obstacle walk is stated once: the checker's source and the pick's both take it from the header
    for name in ("rp_check.hip", "rp_pick.hip"):
        text = open(os.path.join(P.CSRC, name)).read()
        assert '#include "rp_check_rules.h"' in text and "obb_obb(" not in text and "merge_swept(" not in text, name
    # ... and so is the lift step: the lifter's source and the pick's compile the same text of the walk and the same rules
    for name in ("rp_lift.hip", "rp_pick.hip"):
        text = open(os.path.join(P.CSRC, name)).read()
        assert '#include "rp_lift_rules.h"' in text and text.count('#include "rp_lift_walk.inc"') == 1, name
        assert "rp_sincos(" not in text and "rp_atan(" not in text and "find_segment" not in text.replace("find_segment(row, tb.n_seg, tb.iters, s)", ""), name


# ---- the pin: the reference planner's own decision -------------------------------------------------------------------------------
def test_pin_is_the_planners_decision_on_arc_hv_l1_draw():
    """All 120 stored blocks of the fixture, over the N + 1 = 21 poses its rows carry: reasons, the 27 feasible, their 25 hits, the
    winner 92, its cost and the 25 collisions in front of it are the fixture's."""
    c = P.pin()
    f, e, r = c.fixture, c.extras, c.ref
    assert c.planes[0].shape == (120, 21) and c.mode == P.POSES and c.lengths is None
    ob = c.obs
    assert (len(ob.static_obb), len(ob.static_tri), len(ob.static_circ), ob.dyn_obb.shape[0]) == (1, 1, 1, 2)
    np.testing.assert_array_equal(r.lift.status >> 4 & 7, f.reason)
    feas = r.lift.status == 1
    assert r.n_feasible == 27 == len(f.index) - e.n_infeasible_kinematics
    np.testing.assert_array_equal((r.first_pose_hit >= 0)[feas], e.collide_all[feas] > 0)
    assert r.n_collision == 25 and (r.first_pose_hit[~feas] == -1).all() and (r.first_segment_hit == -1).all()
    assert r.best == 92 and int(f.index[r.best]) == e.winner
    print(f"pin: best_cost {r.best_cost!r} against the fixture's {e.winner_cost!r}")
    assert abs(r.best_cost - e.winner_cost) <= S.COST_RTOL * e.winner_cost
    assert r.n_collision_before_best == 25 == e.n_infeasible_collision
    np.testing.assert_array_equal(r.reason_counts, np.bincount(f.reason, minlength=8) * (np.arange(8) > 0))
    np.testing.assert_array_equal(r.status[feas & (r.first_pose_hit >= 0)] & 0xFF, 3)
    np.testing.assert_array_equal(r.status[feas & (r.first_pose_hit >= 0)] >> 8, r.first_pose_hit[feas & (r.first_pose_hit >= 0)])
    # the winner's block is the fixture's stored block: the inputs over all 21 poses, the lifted rows over the trajectory's own length
    # to the lift's tolerances (behind it the reference extends Cartesian and curvilinear rows by different rules, tests/test_score_abi.py)
    block, stored, own = r.best_states, f.states[r.best], int(f.lengths[r.best])
    assert own < 21
    for row in range(14):
        if row in P.INPUT_ROWS:
            np.testing.assert_array_equal(block[row], stored[row])
        else:
            assert np.abs(block[row] - stored[row])[:own].max() <= (L.TOL if row in (0, 1, 2, L.RP_THETA_CL) else L.STATE_ATOL), row


def test_pin_hits_and_winner_cost_on_arc_hv_l2_obs():
    """48 of that plan's 540 blocks are stored: hits and the winner's cost are pinned, the counts are not."""
    c = P.pin("arc_hv_l2_obs")
    f, e, r = c.fixture, c.extras, c.ref
    feas = r.lift.status == 1
    np.testing.assert_array_equal(r.lift.status >> 4 & 7, f.reason)
    np.testing.assert_array_equal((r.first_pose_hit >= 0)[feas], e.collide_all[feas] > 0)
    assert 5 <= r.n_collision <= r.n_feasible - 5
    assert int(f.index[r.best]) == e.winner and abs(r.best_cost - e.winner_cost) <= S.COST_RTOL * e.winner_cost


# ---- the conditions the GPU tests rest on --------------------------------------------------------------------------------------
def _all_cases():
    yield P.pin()
    for name in P.CASES:
        yield P.case(name)


def test_no_first_hit_and_no_winner_of_a_gpu_case_hangs_on_the_last_bits():
    for c in _all_cases():
        steady, gap = P.knife_edges(c)
        print(f"{c.name}: first hits steady under +-{P.EDGE:g} m: {steady}; smallest relative cost gap to the winner {gap:.1e}")
        assert steady and gap >= P.COST_GAP, c.name
    steady, gap = P.knife_edges(P.pin("arc_hv_l2_obs"))
    assert steady and gap >= P.COST_GAP


def test_no_kinematic_verdict_of_a_gpu_case_hangs_on_the_last_bits():
    for c in _all_cases():
        worst, flips = L.knife_edge(c.p, c.ref.lift)
        print(f"{c.name}: margin {worst:.2e}, rounding flips {flips}")
        assert worst >= L.MARGIN and flips == 0, c.name


def test_reference_selection_on_small_tables():
    """The plain-Python selection itself: ties go to the smaller index, a NaN cost never wins, colliding trajectories count in front
    of the winner in (cost, k) order, all of them without one."""
    st = np.array([1, 3, 1, 3, 2, 3, 1], np.uint32)
    assert P.select(st, np.array([5.0, 1.0, 5.0, 5.0, np.nan, 9.0, np.nan])) == (0, 1)
    assert P.select(st, np.array([7.0, 1.0, 5.0, 5.0, np.nan, 9.0, 2.0])) == (6, 1)
    assert P.select(st, np.array([7.0, 1.0, 5.0, 5.0, np.nan, 9.0, 5.0])) == (2, 1)
    assert P.select(st, np.array([7.0, 1.0, 5.0, 5.0, np.nan, 9.0, np.nan]))[0] == 2
    assert P.select(np.array([3, 2, 3], np.uint32), np.array([1.0, np.nan, 2.0])) == (-1, 2)
    assert P.select(np.array([1, 3], np.uint32), np.array([np.nan, 2.0])) == (-1, 1)
    assert P.select(np.array([3, 1], np.uint32), np.array([4.0, 4.0])) == (1, 1) and P.select(np.array([1, 3], np.uint32), np.array([4.0, 4.0])) == (0, 0)


def test_cases_contain_what_their_names_say():
    out = {name: P.case(name) for name in P.CASES}
    for name, c in out.items():
        K, n = P.CASES[name]
        r = c.ref
        assert c.planes[0].shape == (K, n), name
        assert r.n_feasible - r.n_collision == int((r.status == 1).sum()) and r.n_collision >= r.n_collision_before_best, name
        assert (r.best >= 0) == bool((r.status == 1).any()) and (r.best_states is None) == (r.best < 0), name
        np.testing.assert_array_equal(r.first_pose_hit[r.lift.status != 1], -1)
        np.testing.assert_array_equal(r.first_segment_hit[r.lift.status != 1], -1)
    # chunk boundaries: the first hit is pose 62 (the last of 63), pose 63, pose 64 with segment 63 -- the pair that crosses a chunk --
    # and pose 128 with segment 127
    hit = lambda name, k: (int(out[name].ref.first_pose_hit[k]), int(out[name].ref.first_segment_hit[k]))   # noqa: E731
    assert hit("n63", 1) == (62, 61) and hit("n63", 0) == (-1, -1) and out["n63"].ref.best == 0
    assert hit("n64", 0) == (63, 62) and hit("n64", 1) == (-1, -1) and out["n64"].ref.best == 1
    assert hit("n65", 0) == (64, 63) and hit("n65", 1) == (-1, -1) and out["n65"].ref.best == 1
    assert hit("n129", 0) == (128, 127) and hit("n129", 1) == (-1, -1) and out["n129"].ref.best == 1
    for name in ("n63", "n64", "n65", "n129"):
        assert out[name].mode == P.POSES | P.SWEPT and out[name].ref.n_feasible == 2 and out[name].ref.n_collision == 1
        assert int(out[name].ref.status[out[name].ref.first_pose_hit >= 0][0]) == S.status_word(3, 0, int(out[name].ref.first_pose_hit.max()))
    c = out["ragged"]
    assert sorted(c.lengths)[0] == 1 and max(c.lengths) == 65 and c.ref.best > 0 and 5 <= c.ref.n_collision <= c.ref.n_feasible - 5
    one = np.flatnonzero((c.lengths == 1) & (c.ref.lift.status == 1))
    assert one.size and (c.ref.first_segment_hit[one] == -1).all()   # a length-1 trajectory has no segment
    c = out["many"]
    assert c.ref.best > 1024 and c.ref.n_collision_before_best > 64 and c.ref.n_collision > c.ref.n_collision_before_best
    assert c.ref.n_feasible - c.ref.n_collision >= 10 and len(c.ref.status) - c.ref.n_feasible >= 100
    c = out["factor3"]
    first, end = c.obs.dyn_t0, c.obs.dyn_t0 + c.obs.dyn_obb.shape[1]
    n = P.CASES["factor3"][1]
    assert c.p.factor == 3 and c.p.time_step0 < first and end - 1 < c.p.time_step0 + (n - 2) < c.p.time_step0 + (n - 1) * 3
    np.testing.assert_array_equal(c.ref.first_pose_hit, [4, -1, -1, -1, 8, -1, -1, -1])      # poses: time_step0 + i * factor
    np.testing.assert_array_equal(c.ref.first_segment_hit, [-1, 10, 1, -1, -1, -1, -1, -1])   # segments: time_step0 + i
    assert int(c.ref.status[1]) == S.status_word(3, 0, 10) and int(c.ref.status[0]) == S.status_word(3, 0, 4) and c.ref.lift.status[3] != 1
    with_factor_1 = P.first_hits(P._params(c.p, factor=1), c.path, c.obs, c.ref.lift, c.mode)
    assert not np.array_equal(with_factor_1[0], c.ref.first_pose_hit) and np.array_equal(with_factor_1[1], c.ref.first_segment_hit)
    c = out["standstill"]
    still = (np.abs(c.planes[1]) < S.EPS) | (c.planes[1] <= 0.001)
    assert still[:, 60:71].all() and not still[:, :60].any() and not still[:, 71:].any() and c.theta0 is not None
    o = c.ref.lift
    assert (o.theta[:, 60:71] == o.theta[:, 59:60]).all() and c.ref.n_feasible == 4
    np.testing.assert_array_equal(c.ref.first_pose_hit, [65, -1, 65, -1])
    follows_path = o.theta.copy()
    follows_path[:, 60:71] -= o.theta_cl[:, 60:71]   # the orientation the path has there: with it nothing is hit
    assert (P.first_hits(c.p, c.path, c.obs, o, c.mode, theta=follows_path)[0] == -1).all()
    c = out["low_vel"]
    assert c.p.low_vel_mode == 1 and 1 <= c.ref.n_collision < c.ref.n_feasible < 8
    c = out["long_path"]
    assert len(c.path.pos) - 1 == P.LF_LDS_ROWS + 1 and 1 <= c.ref.n_collision < c.ref.n_feasible
    assert len(L.fixture_path("cfg2_ref_draw").pos) - 1 <= P.LF_LDS_ROWS
    c = out["many_static"]
    ob = c.obs
    assert len(ob.static_obb) + len(ob.static_tri) + len(ob.static_circ) == P.CK_LDS_ROWS + 1 and 1 <= c.ref.n_collision < c.ref.n_feasible
    assert all(len(out[name].obs.static_circ) <= P.CK_LDS_ROWS for name in ("many", "all_collide", "duplicates"))
    c = out["all_infeasible"]
    assert c.ref.n_feasible == 0 and c.ref.best == -1 and math.isnan(c.ref.best_cost) and c.ref.reason_counts.sum() == 5
    c = out["all_collide"]
    assert c.ref.best == -1 and c.ref.n_collision_before_best == c.ref.n_collision == c.ref.n_feasible == 4 and c.ref.best_states is None
    for name in ("no_obstacles", "mode0"):
        c = out[name]
        feas = c.ref.lift.status == 1
        assert c.ref.n_collision == 0 and c.ref.best == int(np.flatnonzero(feas)[np.argmin(c.ref.cost[feas])])
    assert out["no_obstacles"].obs is None and out["mode0"].mode == 0 and len(out["mode0"].obs.static_circ) > 0
    for q in range(6):
        np.testing.assert_array_equal(out["mode0"].planes[q], out["all_collide"].planes[q])
    c = out["duplicates"]
    for q in c.planes:
        assert np.array_equal(q[2], q[5]) and np.array_equal(q[1], q[6])
    assert c.ref.best == 2 and c.ref.cost[5] == c.ref.cost[2] and c.ref.status[5] == 1
    assert c.ref.cost[1] == c.ref.cost[6] < c.ref.best_cost and c.ref.n_collision_before_best == 2 == c.ref.n_collision
