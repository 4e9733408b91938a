"""librp_score.so exports what include/rp_score.h declares and what the binding of commonroad_rp_amd.trajectory_score binds -- no
more, no less; the header stands on its own; without the library or without a GPU a TrajectoryScorer fails loudly.  Then, on the
CPU alone, the NumPy reference of tests/_score.py pinned to the draw fixtures, to oracle.frontend.project and to the tie rule, and the
conditions the GPU tests of tests/test_score.py rest on.  No compute calls on the device here."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, clearance, ensemble_check, trajectory_check, trajectory_score
from oracle import frontend

import _score as R

REPO = R.REPO
HEADER = R.HEADER
SOURCE = R.SOURCE
CSRC = os.path.dirname(SOURCE)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared_functions():
    return sorted(set(re.findall(r"\b(rp_[a-z_]+)\s*\(", _header())))


def _library():
    paths = (trajectory_score.LIB_PATH, clearance.LIB_PATH, ensemble_check.LIB_PATH, trajectory_check.LIB_PATH, _capi.LIB_PATH)
    if not all(os.path.exists(p) for p in paths):
        import __graft_entry__
        __graft_entry__.build()
    return trajectory_score.LIB_PATH


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    declared = _declared_functions()
    assert declared == sorted(trajectory_score.EXPORTED_SYMBOLS)
    assert len(declared) == 7 and all(name.startswith("rp_score_") for name in declared)
    assert not any(ch.isdigit() for name in declared for ch in name)
    assert _exported(_library()) == declared
    # the other four libraries are what they were: nothing of the scorer went into them, and nothing of theirs is exported here
    for other in (_capi.EXPORTED_SYMBOLS, trajectory_check.EXPORTED_SYMBOLS, ensemble_check.EXPORTED_SYMBOLS, clearance.EXPORTED_SYMBOLS):
        assert not any(name.startswith("rp_score") for name in other)
        assert not set(other) & set(declared)
    for lib in (_capi.LIB_PATH, trajectory_check.LIB_PATH, ensemble_check.LIB_PATH, clearance.LIB_PATH):
        assert not any(name.startswith("rp_score") for name in _exported(lib)), lib


def test_abi_version_limits_and_package_exports():
    lib = trajectory_score.load_library(_library())
    assert lib.rp_score_abi_version() == trajectory_score.ABI_VERSION == 1
    assert commonroad_rp_amd.TrajectoryScorer is trajectory_score.TrajectoryScorer
    assert commonroad_rp_amd.TrajectoryScoreResult is trajectory_score.TrajectoryScoreResult
    src = _header()
    assert int(re.search(r"#define\s+RP_SCORE_ABI_VERSION\s+(\d+)", src).group(1)) == 1
    assert int(re.search(r"#define\s+RP_SCORE_MAX_POSES\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", src).group(1)) == 24
    assert trajectory_score.MAX_POSES == clearance.MAX_POSES == 1 << 24          # capped like RP_CLEARANCE_MAX_POSES
    assert int(re.search(r"#define\s+RP_SCORE_EXHAUSTIVE\s+\(1u\s*<<\s*(\d+)\)", src).group(1)) == 0 and trajectory_score.EXHAUSTIVE == 1
    assert [f.name for f in __import__("dataclasses").fields(trajectory_score.TrajectoryScoreResult)] == [
        "status", "cost", "best", "best_cost", "n_feasible", "reason_counts", "s", "d", "theta_cl"]
    for name in ("set_reference", "project", "score", "score_states"):
        assert callable(getattr(trajectory_score.TrajectoryScorer, name))


def test_header_compiles_on_its_own(tmp_path):
    body = ("int uses(rp_score *c, const rp_params *p, const rp_cost *q, int64_t *b, double *bc, int64_t *nf, int64_t *rc) {\n"
            "  return rp_score_evaluate(c, p, q, 0, 1, 0, 0, 0, 0, 0, 0, 0, RP_SCORE_EXHAUSTIVE, 0, 0, 0, 0, 0, b, bc, nf, rc)\n"
            "         + rp_score_project(c, 0, 0, 0, 0, 0, 0, nf) + rp_score_set_reference(c, 0, 0, 0, 0, 20.0)\n"
            "         + (RP_SCORE_MAX_POSES >= ((int64_t)1 << 24) ? 0 : 1) + RP_EINVAL; }\n")
    for name, includes in (("only_rp_score", '#include "rp_score.h"   /* first and only: the header must be self-contained */\n'),
                           ("score_then_others", '#include "rp_score.h"\n#include "rp_check.h"\n#include "rp_ensemble.h"\n#include "rp_clearance.h"\n'),
                           ("others_then_score", '#include "rp_check.h"\n#include "rp_ensemble.h"\n#include "rp_clearance.h"\n#include "rp_score.h"\n')):
        src = tmp_path / f"{name}.c"
        src.write_text(includes + body)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / f"{name}.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        trajectory_score.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        trajectory_score.TrajectoryScorer(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        trajectory_score.TrajectoryScorer(0)


def test_makefile_targets_and_source_hash_inputs_untouched():
    src = open(SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "asm" not in re.sub(r"//.*", "", src)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1)
    assert "score" not in srcs
    assert re.search(r"^all:.*\$\(SCORELIB\)", mk, flags=re.M) and re.search(r"^score-resource-usage:", mk, flags=re.M)
    assert re.search(r"^\$\(SCORELIB\): rp_score\.hip ", mk, flags=re.M)
    # the files behind rp_source_hash() and the three sibling libraries are only included: the scorer defines nothing in them
    # (nor in what the libraries' host sides and bindings share)
    for name in srcs.split() + ["rp_check.hip", "rp_ensemble.hip", "rp_clearance.hip", "rp_session.h", "rp_obstacle_tables.h", "../commonroad_rp_amd/_session.py"]:
        text = open(os.path.join(CSRC, name)).read()
        assert "rp_score" not in text and "SC_LDS_ROWS" not in text, name
    if os.path.isdir(os.path.join(REPO, ".git")):
        files = [os.path.join("commonroad-reactive-planner_amd", "csrc", n) for n in srcs.split() + ["rp_check.hip", "rp_ensemble.hip", "rp_clearance.hip"]]
        try:
            out = subprocess.run(["git", "diff", "--stat", "HEAD", "--"] + [os.path.normpath(f) for f in files], cwd=REPO, capture_output=True,
                                 text=True, timeout=60)
        except (OSError, subprocess.TimeoutExpired):
            out = None
        if out is not None and out.returncode == 0:
            assert out.stdout.strip() == "", out.stdout


# ---- the reference, pinned -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.DRAW_FIXTURES)
def test_reference_round_trip_verdicts_and_costs_on_draw_fixtures(name):
    """The fixture's own Cartesian rows, projected, give back its curvilinear rows; the transcribed constraints give its reasons; the
    cost of the projected rows is its cost.

    Only steps i < traj_len of a block are compared, BY DESIGN: beyond a candidate's own length the reference's ``enlarge`` extends the
    Cartesian rows (constant heading, integrated speed) and the curvilinear rows (s integrated, d and theta_cl held) by different
    rules, so the extension does not round-trip (cfg1_ref_l1_draw: up to 0.78 m in d there).  Costs are therefore compared for the
    feasible blocks with traj_len == N + 1 alone.  Measured over all valid steps of all thirteen fixtures: s 1.4e-14 m, d 2.2e-15 m,
    theta_cl 8.3e-16 rad, cost 3.5e-15 relative, 0 of 997 reasons different."""
    f, o = R.fixture(name), R.fixture_reference(name)
    assert not np.isnan(o.s[o.valid]).any()
    worst = [float(np.abs(got - f.states[:, row])[o.valid].max()) for got, row in ((o.s, R.RP_S), (o.d, R.RP_D), (o.theta_cl, R.RP_THETA_CL))]
    print(f"{name}: s {worst[0]:.1e} m, d {worst[1]:.1e} m, theta_cl {worst[2]:.1e} rad over {int(o.valid.sum())} steps")
    assert max(worst) <= R.TOL
    assert np.isnan(o.s[~o.valid]).all() and np.isnan(o.theta_cl[~o.valid]).all()
    np.testing.assert_array_equal((o.status >> 4) & 7, f.reason)
    np.testing.assert_array_equal((o.status & 3) == 1, f.reason == 0)
    full = (o.status == 1) & (f.lengths == f.n)
    if name in ("cfg2_ref_draw", "cfg3_ref_draw"):
        assert int(full.sum()) == (4 if name == "cfg2_ref_draw" else 2)
    if full.any():
        rel = np.abs(o.cost[full] - f.fixture_cost[full]) / np.abs(f.fixture_cost[full])
        print(f"{name}: cost {rel.max():.1e} relative over {int(full.sum())} blocks")
        assert rel.max() <= R.COST_RTOL


def test_reference_reasons_cover_the_fixture_kinds():
    seen = set()
    total = 0
    for name in R.DRAW_FIXTURES:
        seen |= set(int(r) for r in R.fixture(name).reason)
        total += len(R.fixture(name).reason)
    assert {0, 2, 3, 4, 5} <= seen and total >= 900


def test_vectorised_projection_is_oracle_frontend_project_point_by_point():
    """tests/_score.py turns the point loop of oracle.frontend.project into array operations; here the two are held together point by
    point: inside / outside agree, s and d agree to 1e-12 m (the scalar function sums its products through ``@``)."""
    rng = np.random.default_rng(5)
    checked = outside = 0
    for kind, d_limit in (("cfg2", 20.0), ("u", 20.0), ("u", 1.5), ("two_vertex", 3.0), ("at_cap", 20.0)):
        ref, pos, _ = R.path(kind)
        lo, hi = ref.min(0) - 6.0, ref.max(0) + 6.0
        pts = rng.uniform(lo, hi, (60, 2))
        s, d, seg, _ = R.project_batch(ref, pos, pts[:, 0], pts[:, 1], d_limit)
        for q in range(len(pts)):
            want = frontend.project(ref, pos, pts[q, 0], pts[q, 1], d_limit)
            checked += 1
            if want is None:
                outside += 1
                assert seg[q] == -1 and math.isnan(s[q]) and math.isnan(d[q])
            else:
                assert seg[q] >= 0 and abs(s[q] - want[0]) <= 1e-12 and abs(d[q] - want[1]) <= 1e-12, (kind, q)
                assert pos[seg[q]] - 1e-12 <= s[q] <= pos[seg[q] + 1] + 1e-12
    assert checked == 300 and 10 <= outside <= 200
    for name in ("cfg2_ref_draw", "scurve_lv_l1_draw"):   # ... and on fixture poses
        f, o = R.fixture(name), R.fixture_reference(name)
        for k in range(0, len(f.index), 9):
            for i in range(0, int(f.lengths[k]), 5):
                want = frontend.project(f.ref, f.ref_pos, f.states[k, R.RP_X, i], f.states[k, R.RP_Y, i], f.d_limit)
                assert abs(o.s[k, i] - want[0]) <= 1e-12 and abs(o.d[k, i] - want[1]) <= 1e-12


def test_tie_rule_on_the_u_path():
    """(4, 2) lies at |d| = 2.0 exactly on the first and on the last segment of the U: the first wins.  Both functions say so."""
    ref, pos, _ = R.path("u")
    np.testing.assert_array_equal(ref, R.U_PATH)
    s, d, seg, _, cand_ad, cand_s = R.project_batch(ref, pos, [4.0], [2.0], keep_candidates=True)
    assert (s[0], d[0], seg[0]) == (4.0, 2.0, 0)
    assert sorted(cand_ad[~np.isnan(cand_ad)])[:2] == [2.0, 2.0] and (cand_ad == 2.0).sum() == 2   # the two nearest candidates tie exactly
    assert sorted(cand_s[cand_ad == 2.0]) == [4.0, pytest.approx(33.65685424949238, abs=1e-12)]
    assert frontend.project(ref, pos, 4.0, 2.0) == (4.0, 2.0)
    assert R.project_batch(ref, pos, [4.0], [2.0], 1.5)[2][0] == -1 and frontend.project(ref, pos, 4.0, 2.0, 1.5) is None
    s, d, seg, _ = R.project_batch(ref, pos, [4.0], [3.0])
    assert seg[0] == 5 and d[0] == 1.0 and s[0] == pytest.approx(16.0 + 4.0 * math.sqrt(2.0) + 12.0, abs=1e-12)
    assert s[0] == pytest.approx(33.6568, abs=1e-4)


def test_reference_selection_and_ordering_rules():
    """A later kinematic failure decides over an earlier pose outside the domain; the cost's middle entry is v[len // 2]; a NaN pose is
    outside the domain."""
    f = R.fixture("cfg2_ref_draw")
    k = int(np.flatnonzero((R.fixture_reference("cfg2_ref_draw").status == 1) & (f.lengths == f.n))[0])
    rows = {q: r[k:k + 1].copy() for q, r in R.fixture_rows(f).items() if q != "lengths"}
    base = R.reference(f.p, f.cost, f.ref, f.ref_pos, f.ref_theta, **rows)
    assert base.status[0] == 1 and base.best == 0
    rows["x"][0, 5] = math.nan
    out = R.reference(f.p, f.cost, f.ref, f.ref_pos, f.ref_theta, **rows)
    assert out.status[0] == R.status_word(2, R.OUT_OF_DOMAIN, 5) and math.isnan(out.cost[0]) and out.best == -1 and out.reason_counts[6] == 1
    rows["a"][0, 20] = 100.0
    out = R.reference(f.p, f.cost, f.ref, f.ref_pos, f.ref_theta, **rows)
    assert out.status[0] == R.status_word(2, R.REASON["acceleration"], 20)
    v = np.arange(7.0)
    c = _capi.make_cost(desired_speed=0.0)
    zero = np.zeros(7)
    assert R.cost_of(c, zero, v, zero, zero, zero) == 25.0 * (v ** 2).sum() + 50.0 * 36.0 + 100.0 * 9.0   # middle entry v[7 // 2] = 3


# ---- the conditions the GPU tests rest on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.SHAPES])
def test_shape_inputs_have_no_near_ties_and_keep_their_lateral_range(name):
    c = R.shape_case(name)
    o = c.ref_out
    assert R.near_ties(c.ref, c.ref_pos, c.x, c.y, c.d_limit) == 0
    assert not np.isnan(o.s[o.valid]).any() and np.abs(o.d[o.valid]).max() <= c.lateral + 1e-9
    if c.lateral > 3.0:
        assert np.abs(o.d[o.valid]).min() >= 12.0
    n_seg = len(c.ref) - 1
    assert n_seg == {"one_segment": 1, "lds_cap": R.LDS_ROWS, "lds_cap_plus_one": R.LDS_ROWS + 1, "far_lds": R.LDS_ROWS,
                     "far_device_memory": R.LDS_ROWS + 1}.get(name, n_seg)
    if c.lateral > 3.0:   # more open segments than the eight a lane lists: the bound at the pose's own |d| admits them
        centre, radius = 0.5 * (c.ref[1:] + c.ref[:-1]), 0.5 * np.linalg.norm(c.ref[1:] - c.ref[:-1], axis=1)
        dist = np.hypot(c.x[o.valid][:, None] - centre[None, :, 0], c.y[o.valid][:, None] - centre[None, :, 1])
        assert ((dist <= radius[None] + np.abs(o.d[o.valid])[:, None]).sum(1) > 8).any()


def test_shape_inputs_fail_every_check_somewhere_and_fixture_inputs_have_no_near_ties():
    counts = sum(R.shape_case(c[0]).ref_out.reason_counts for c in R.SHAPES)
    assert (counts[1:6] > 0).all(), counts
    assert sum(R.shape_case(c[0]).ref_out.n_feasible for c in R.SHAPES) >= 100
    for name in R.GPU_FIXTURES:
        f = R.fixture(name)
        valid = R.fixture_reference(name).valid
        assert R.near_ties(f.ref, f.ref_pos, f.states[:, R.RP_X][valid], f.states[:, R.RP_Y][valid], f.d_limit) == 0, name
