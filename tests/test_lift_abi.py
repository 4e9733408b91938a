"""librp_lift.so exports what include/rp_lift.h declares and what the binding of commonroad_rp_amd.lift binds -- no more, no less; the
header stands on its own; without the library or without a GPU a TrajectoryLifter fails loudly.  Then, on the CPU alone, the NumPy
reference of tests/_lift.py pinned to the draw fixtures and to CoordinateSystem.convert_to_cartesian_coords, and the conditions the
GPU tests of tests/test_lift.py rest on.  No compute calls on the device here."""
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, clearance, ensemble_check, lift, trajectory_check, trajectory_score
from commonroad_rp_amd.coordinate_system import CoordinateSystem

import _lift as R
import _score as S

REPO = R.REPO
CSRC = os.path.dirname(R.SOURCE)
SIBLINGS = (_capi, trajectory_check, ensemble_check, clearance, trajectory_score)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(R.HEADER).read(), flags=re.S)


def _library():
    if not all(os.path.exists(m.LIB_PATH) for m in SIBLINGS + (lift,)):
        import __graft_entry__
        __graft_entry__.build()
    return lift.LIB_PATH


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    declared = sorted(set(re.findall(r"\b(rp_[a-z_]+)\s*\(", _header())))
    assert declared == sorted(lift.EXPORTED_SYMBOLS)
    assert len(declared) == 7 and all(name.startswith("rp_lift_") for name in declared)
    assert _exported(_library()) == declared
    # the other five libraries are what they were: nothing of the lift went into them, and nothing of theirs is exported here
    for m in SIBLINGS:
        assert not any(name.startswith("rp_lift") for name in m.EXPORTED_SYMBOLS)
        assert not set(m.EXPORTED_SYMBOLS) & set(declared)
        assert not any(name.startswith("rp_lift") for name in _exported(m.LIB_PATH)), m.LIB_PATH


def test_abi_version_limits_and_package_exports():
    lib = lift.load_library(_library())
    assert lib.rp_lift_abi_version() == lift.ABI_VERSION == 1
    assert commonroad_rp_amd.TrajectoryLifter is lift.TrajectoryLifter
    assert commonroad_rp_amd.TrajectoryLiftResult is lift.TrajectoryLiftResult
    src = _header()
    assert int(re.search(r"#define\s+RP_LIFT_ABI_VERSION\s+(\d+)", src).group(1)) == 1
    assert int(re.search(r"#define\s+RP_LIFT_MAX_POSES\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", src).group(1)) == 24
    assert lift.MAX_POSES == trajectory_score.MAX_POSES == 1 << 24
    assert [f.name for f in dataclasses.fields(lift.TrajectoryLiftResult)] == [
        "status", "first_feasible", "n_feasible", "reason_counts", "x", "y", "theta", "v", "a", "kappa", "kappa_dot", "theta_cl"]
    for name in ("set_reference", "points", "lift", "lift_states", "close", "__enter__", "__exit__"):
        assert callable(getattr(lift.TrajectoryLifter, name))
    for name in ("label", "reason", "step"):
        assert isinstance(getattr(lift.TrajectoryLiftResult, name), property)
    # the header states the on-path rule and that the reference's wrap-around index is not kept
    text = open(R.HEADER).read()
    assert "THE SEGMENT AND ON-PATH RULE" in text and "QUIRK IS NOT KEPT" in text


def test_header_compiles_on_its_own(tmp_path):
    body = ("int uses(rp_lift *c, const rp_params *p, int64_t *ff, int64_t *nf, int64_t *rc) {\n"
            "  return rp_lift_evaluate(c, p, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0u, 0, 0, 0, 0, 0, 0, 0, 0, 0, ff, nf, rc)\n"
            "         + rp_lift_points(c, 0, 0, 0, 0, 0, 0, nf) + rp_lift_set_reference(c, 0, 0, 0, 0, 0, 0, 20.0)\n"
            "         + (RP_LIFT_MAX_POSES >= ((int64_t)1 << 24) ? 0 : 1) + RP_EINVAL + RP_LIFT_ABI_VERSION; }\n")
    others = '#include "rp_check.h"\n#include "rp_ensemble.h"\n#include "rp_clearance.h"\n#include "rp_score.h"\n'
    for name, includes in (("only_rp_lift", '#include "rp_lift.h"   /* first and only: the header must be self-contained */\n'),
                           ("lift_then_others", '#include "rp_lift.h"\n' + others), ("others_then_lift", others + '#include "rp_lift.h"\n')):
        src = tmp_path / f"{name}.c"
        src.write_text(includes + body)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / f"{name}.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        lift.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        lift.TrajectoryLifter(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        lift.TrajectoryLifter(0)


def test_makefile_targets_and_source_hash_inputs_untouched():
    src = open(R.SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "asm" not in re.sub(r"//.*", "", src)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1)
    assert "lift" not in srcs
    assert re.search(r"^all:.*\$\(LIFTLIB\)", mk, flags=re.M) and re.search(r"^lift-resource-usage:", mk, flags=re.M)
    assert re.search(r"^\$\(LIFTLIB\): rp_lift\.hip rp_device\.h rp_math\.h rp_frontend\.h \.\./\.\./include/rp_lift\.h \.\./\.\./include/rp_amd\.h$", mk, flags=re.M)
    assert re.search(r"^clean:\n\trm -f .*\$\(LIFTLIB\)", mk, flags=re.M)
    # the files behind rp_source_hash() and the four sibling libraries are only included: the lift defines nothing in them
    # (nor in what the libraries' host sides and bindings share)
    for name in srcs.split() + ["rp_check.hip", "rp_ensemble.hip", "rp_clearance.hip", "rp_score.hip", "rp_session.h", "rp_obstacle_tables.h", "../commonroad_rp_amd/_session.py"]:
        text = open(os.path.join(CSRC, name)).read()
        assert "rp_lift" not in text and "LF_LDS_ROWS" not in text, name


# ---- the reference, pinned -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PINNED_FIXTURES)
def test_reference_gives_back_the_fixture_rows_and_reasons(name):
    """Rows 7, 8 and 10 .. 13 of every stored trajectory, lifted over its own length, give back rows 0 .. 5 and 9 to 1e-12; row 6 is the
    first difference of row 5; reason and label are the fixture's.  Beyond a trajectory's own length the stored rows are the reference's
    horizon extension, which the lift does not make."""
    f, o = S.fixture(name), R.fixture_reference(name)
    valid = np.arange(f.n)[None, :] < f.lengths[:, None]
    worst = {pl: float(np.abs(getattr(o, pl) - f.states[:, row])[valid].max()) for pl, row in
             (("x", 0), ("y", 1), ("theta", 2), ("v", 3), ("a", 4), ("kappa", 5), ("theta_cl", R.RP_THETA_CL))}
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    assert not any(np.isnan(getattr(o, pl)[valid]).any() for pl in R.PLANES)
    assert max(worst.values()) <= 1e-12
    diff = np.concatenate((np.zeros((len(f.index), 1)), np.diff(f.states[:, 5], axis=1)), 1)
    assert np.abs(o.kappa_dot - diff)[valid].max() <= 1e-12 and np.abs(f.states[:, R.RP_KAPPA_DOT] - diff)[valid].max() <= 1e-12
    assert all(np.isnan(getattr(o, pl)[~valid]).all() for pl in R.PLANES)
    np.testing.assert_array_equal((o.status >> 4) & 7, f.reason)
    # (the fixture's label 3 is a kinematically feasible trajectory that collides: the lift knows no obstacles)
    np.testing.assert_array_equal(o.status & 3, np.where(f.label == 3, 1, f.label))
    np.testing.assert_array_equal((o.status & 3) == 1, f.reason == 0)


def test_reference_reasons_cover_the_kinds_and_the_modes():
    seen = set()
    for name in R.PINNED_FIXTURES:
        seen |= set(int(r) for r in S.fixture(name).reason)
    assert {0, 2, 3, 4, 5} <= seen
    assert S.fixture("scurve_lv_l1_draw").p.low_vel_mode == 1 and S.fixture("arc_hv_standstill_draw").p.low_vel_mode == 0
    for name in ("arc_hv_standstill_draw", "scurve_lv_l1_draw"):   # the 24 trajectories each with poses at a standstill
        f = S.fixture(name)
        valid = np.arange(f.n)[None, :] < f.lengths[:, None]
        assert int(((f.states[:, R.RP_S_DOT] <= 0.001) & valid).any(axis=1).sum()) == 24


def test_reference_leaves_the_path_where_short_path_ood_does():
    """short_path_ood_draw runs past the end of its path: the reference stops those trajectories at the pose whose s is off the path
    (the one fixture whose reasons are NOT pinned: the reference planner's wrap-around table index decides one of them otherwise)."""
    name = "short_path_ood_draw"
    f, t = S.fixture(name), R.fixture_path(name)
    o = R.reference(f.p, t, **R.fixture_inputs(name))
    valid = np.arange(f.n)[None, :] < f.lengths[:, None]
    off = ((f.states[:, R.RP_S] > t.pos[-1]) | (f.states[:, R.RP_S] < t.pos[0])) & valid
    leaving = off.any(axis=1)
    assert int(leaving.sum()) == 18
    for k in np.flatnonzero(leaving):
        first = int(np.argmax(off[k]))
        assert np.isnan(o.theta[k, first:]).all() and not np.isnan(o.theta[k, :first]).any()
        st = int(o.status[k])
        assert st & 3 == 2 and ((st >> 8) & 0xFFF) <= first and (((st >> 4) & 7) == S.OUT_OF_DOMAIN) == (((st >> 8) & 0xFFF) == first)
    assert not np.isnan(o.theta[~leaving][valid[~leaving]]).any()


def _edge_points(t, rng):
    """s on every vertex, at both ends and just outside them, inside segments; |d| at and just beyond the limit"""
    s = np.concatenate((t.pos, [np.nextafter(t.pos[0], -np.inf), np.nextafter(t.pos[-1], np.inf), t.pos[0] - 1.0, t.pos[-1] + 1.0],
                        rng.uniform(t.pos[0], t.pos[-1], 40)))
    d = rng.uniform(-0.9 * t.d_limit, 0.9 * t.d_limit, s.size)
    d[:len(t.pos):3] = 0.0
    extra_s = rng.uniform(t.pos[0], t.pos[-1], 6)
    extra_d = np.array([t.d_limit, -t.d_limit, np.nextafter(t.d_limit, np.inf), -np.nextafter(t.d_limit, np.inf), 1.5 * t.d_limit, 0.0])
    return np.concatenate((s, extra_s, [t.pos[0], t.pos[-1]])), np.concatenate((d, extra_d, [t.d_limit, -t.d_limit]))


@pytest.mark.parametrize("name", R.PINNED_FIXTURES + ("u_path",))
def test_reference_points_are_convert_to_cartesian_coords(name):
    rng = np.random.default_rng(11)
    if name == "u_path":
        co = CoordinateSystem(S.U_PATH, proj_domain_d_limit=1.5)
        t = R.NS(ref=co.reference, pos=co.ref_pos, theta=co.ref_theta, curv=co.ref_curv, curv_d=co.ref_curv_d, d_limit=1.5, tan=co.vertex_tangents)
    else:
        t = R.fixture_path(name)
        co = CoordinateSystem(t.ref, proj_domain_d_limit=t.d_limit)
    np.testing.assert_array_equal(co.ref_pos, t.pos)
    np.testing.assert_array_equal(co.reference, t.ref)
    s, d = _edge_points(t, rng)
    x, y, seg = R.points(t, s, d)
    outside = 0
    for q in range(s.size):
        want = co.convert_to_cartesian_coords(float(s[q]), float(d[q]))
        if want is None:
            outside += 1
            assert math.isnan(x[q]) and math.isnan(y[q]) and seg[q] == -1
        else:
            assert x[q] == want[0] and y[q] == want[1] and 0 <= seg[q] <= len(t.pos) - 2
            assert t.pos[seg[q]] <= s[q] <= t.pos[seg[q] + 1]
    assert outside == 7   # four s off the ends and three |d| beyond the limit
    assert seg[len(t.pos) - 1] == len(t.pos) - 2 and seg[0] == 0   # the last vertex lies on the last segment


# ---- the conditions the GPU tests rest on --------------------------------------------------------------------------------------
def _all_cases():
    for name in R.GPU_FIXTURES:
        yield name, S.fixture(name).p, R.fixture_reference(name)
    for name in R.CASES:
        c = R.case(name)
        yield name, c.p, c.out


def test_no_verdict_of_a_gpu_case_hangs_on_the_last_bits():
    """Every fixture and synthetic case of tests/test_lift.py: the smallest distance between a checked quantity and its bound, at or
    before the deciding step, is at least 1e-6 (a thousand times the 1e-9 / a million times the 1e-12 the device is expected to differ
    by), and no yaw rate within 2e-5 of its bound has yaw * 1e5 within 1e-3 of a half-integer."""
    for name, p, o in _all_cases():
        worst, flips = R.knife_edge(p, o)
        print(f"{name}: margin {worst:.2e}, rounding flips {flips}")
        assert worst >= R.MARGIN and flips == 0, name
    for name in R.GPU_FIXTURES:
        assert R.knife_edge(S.fixture(name).p, R.fixture_reference(name))[0] >= 2.5e-4, name


def test_mask_sweep_margins():
    f, t = S.fixture("cfg1_ref_l1_draw"), R.fixture_path("cfg1_ref_l1_draw")
    for mask in (0, 1, 2, 4, 8, 16):
        p = _capi.RpParams.from_buffer_copy(f.p)
        p.constraint_mask = mask
        o = R.reference(p, t, **R.fixture_inputs("cfg1_ref_l1_draw"))
        worst, flips = R.knife_edge(p, o)
        assert worst >= R.MARGIN and flips == 0, mask
        if mask == 0:
            assert o.n_feasible == len(o.status)


def test_synthetic_cases_contain_what_their_names_say():
    out = {name: R.case(name) for name in R.CASES}
    for name, c in out.items():
        K, n = R.CASES[name]
        assert c.planes[0].shape == (K, n if n else len(c.path.pos)), name
        if K >= 8:
            assert 5 * c.out.n_feasible >= K and 5 * (K - c.out.n_feasible) >= K, (name, c.out.n_feasible)
    still = lambda c: (np.abs(c.planes[1]) < S.EPS) | (c.planes[1] <= 0.001)   # noqa: E731
    assert out["one_pose"].theta0 is not None and out["one_pose"].planes[0].shape[1] == 1
    assert sorted(out["ragged"].lengths)[0] == 1 and max(out["ragged"].lengths) == 65 and len(set(out["ragged"].lengths.tolist())) > 30
    for name in ("standstill_head", "standstill_head_theta0"):
        c = out[name]
        assert still(c)[:, :7].all() and not still(c)[:, 7:].any() and (c.theta0 is None) == (name == "standstill_head")
        th0 = np.full(4, c.p.x0_orientation) if c.theta0 is None else c.theta0
        assert (c.out.theta[:, :7] == th0[:, None]).all()
    c = out["standstill_across"]
    assert still(c)[:, 60:71].all() and not still(c)[:, :60].any() and not still(c)[:, 71:].any()
    assert (c.out.theta[:, 60:71] == c.out.theta[:, 59:60]).all() and c.out.n_feasible == 2
    assert still(out["standstill_all"]).all() and out["standstill_all"].planes[0].shape == (1, 70)
    c = out["stop_and_go"]
    runs = np.diff(still(c).astype(int), axis=1)
    assert ((runs == 1).sum(1) == 2).all() and ((runs == -1).sum(1) == 2).all() and still(c)[:, 58:65].all()
    c = out["low_vel"]
    assert c.p.low_vel_mode == 1 and still(c)[:, 25:34].all() and {3} <= set(((c.out.status >> 4) & 7).tolist())
    c = out["off_end"]
    leaves = [int(np.argmax(c.planes[0][k] > c.path.pos[-1])) for k in range(4)]
    assert leaves == [9, 16, 23, 0] and not (c.planes[0][3] > c.path.pos[-1]).any()
    assert [int(s) for s in c.out.status[[0, 2]]] == [S.status_word(2, S.OUT_OF_DOMAIN, 9), S.status_word(2, S.OUT_OF_DOMAIN, 23)]
    assert (c.out.status[1] >> 8) & 0xFFF < 16 and (c.out.status[1] >> 4) & 7 != S.OUT_OF_DOMAIN and np.isnan(c.out.x[1, 16:]).all()
    assert not np.isnan(c.out.x[1, :16]).any()
    c = out["off_start"]
    assert [int(s) for s in c.out.status] == [S.status_word(2, S.OUT_OF_DOMAIN, 0), S.status_word(2, S.REASON["velocity"], 0),
                                              S.status_word(2, S.OUT_OF_DOMAIN, 13), 1]
    assert np.isnan(c.out.x[0]).all() and np.isnan(c.out.x[1, 13:]).all() and not np.isnan(c.out.x[1, :13]).any()
    c = out["vertex_hits"]
    np.testing.assert_array_equal(c.planes[0][0], c.path.pos)
    assert not np.isnan(c.out.x).any()
    c = out["beyond_d"]
    assert c.path.d_limit == 3.0 and c.planes[3][3, 0] == 3.0
    assert [int(s) for s in c.out.status[[0, 1, 3]]] == [S.status_word(2, S.OUT_OF_DOMAIN, 7), S.status_word(2, S.OUT_OF_DOMAIN, 5), 1]
    assert (c.out.status[2] >> 8) & 0xFFF == 4 and (c.out.status[2] >> 4) & 7 != S.OUT_OF_DOMAIN
    assert np.isnan(c.out.x[0, 7:]).all() and not np.isnan(c.out.theta[0]).any() and not np.isnan(c.out.x[1, 9:]).any()
    c = out["nan_input"]
    assert [int(s) for s in c.out.status] == [S.status_word(2, S.OUT_OF_DOMAIN, q) for q in (4, 0, 9)]
    assert np.isnan(c.out.v[0, 4:]).all() and not np.isnan(c.out.v[0, :4]).any()
    assert len(out["long_path"].path.pos) == R.LDS_ROWS + 2 and len(out["long_path_at_cap"].path.pos) == R.LDS_ROWS + 1
    for q in range(6):
        np.testing.assert_array_equal(out["long_path"].planes[q], out["long_path_at_cap"].planes[q])
    assert len(R.fixture_path("cfg2_ref_draw").pos) - 1 <= R.LDS_ROWS
    c = out["many"]
    assert c.out.first_feasible > 0 and c.planes[0].shape[0] > 1024
    seen = np.zeros(8, int)
    for c in out.values():
        seen += c.out.reason_counts
    assert (seen[[1, 3, 4, 5, 6]] > 0).all(), seen


def test_round_trip_poses_have_no_near_ties():
    """tests/test_lift.py hands lift_states of cfg2_ref_draw to the scorer: the projection of those poses must not hang on a tie."""
    f, o = S.fixture("cfg2_ref_draw"), R.fixture_reference("cfg2_ref_draw")
    ok = ~np.isnan(o.x)
    assert ok.sum() > 1000 and S.near_ties(f.ref, f.ref_pos, o.x[ok], o.y[ok], f.d_limit) == 0
