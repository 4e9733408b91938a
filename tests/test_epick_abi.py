"""librp_epick.so exports what include/rp_epick.h declares and what the binding of commonroad_rp_amd.ensemble_pick binds -- no more, no
less; the header stands on its own; without the library or without a GPU an EnsemblePicker fails loudly.  Then, on the CPU alone, the
yardstick of tests/_epick.py: with one member it is the yardstick of the pick, with several its counts are the ensemble checker's, its
risk is the ascending sum, and the cases the GPU tests of tests/test_epick.py run hold what those tests rest on.  No compute calls on
the device here."""
import ctypes as C
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, clearance, ensemble_check, ensemble_pick, lift, pick, trajectory_check, trajectory_score

import _ensemble as E
import _epick as EP
import _lift as L
import _pick as P

SIBLINGS = (_capi, trajectory_check, ensemble_check, clearance, trajectory_score, lift, pick)
EXPORTS = ["rp_epick_abi_version", "rp_epick_create", "rp_epick_destroy", "rp_epick_last_error", "rp_epick_select", "rp_epick_set_members",
           "rp_epick_set_reference", "rp_epick_set_static"]
RESULT_FIELDS = ["struct_size", "reserved_", "best", "best_cost", "n_feasible", "n_collision", "n_collision_before_best", "reason_counts", "best_members_hit",
                 "best_risk"]
PROTECTED = ["rp_check.hip", "rp_ensemble.hip", "rp_clearance.hip", "rp_check_rules.h", "rp_lift_rules.h", "rp_lift_walk.inc", "rp_lift.hip", "rp_score.hip",
             "rp_session.h", "rp_obstacle_tables.h", "../commonroad_rp_amd/_session.py"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(EP.HEADER).read(), flags=re.S)


def _library():
    if not all(os.path.exists(m.LIB_PATH) for m in SIBLINGS + (ensemble_pick,)):
        import __graft_entry__
        __graft_entry__.build()
    return ensemble_pick.LIB_PATH


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    declared = sorted(set(re.findall(r"\b(rp_[a-z_0-9]+)\s*\(", _header())))
    assert declared == sorted(ensemble_pick.EXPORTED_SYMBOLS) == EXPORTS
    assert not any(re.search(r"\d", name) or name.startswith("rp_pick") for name in declared)
    assert _exported(_library()) == declared
    # the other seven libraries are what they were: nothing of this one went into them, and nothing of theirs is exported here
    for m in SIBLINGS:
        assert not any(name.startswith("rp_epick") for name in m.EXPORTED_SYMBOLS)
        assert not set(m.EXPORTED_SYMBOLS) & set(declared)
        assert not any(name.startswith("rp_epick") for name in _exported(m.LIB_PATH)), m.LIB_PATH


def test_abi_version_struct_layout_limits_and_package_exports(tmp_path):
    lib = ensemble_pick.load_library(_library())
    assert lib.rp_epick_abi_version() == ensemble_pick.ABI_VERSION == 1
    assert commonroad_rp_amd.EnsemblePicker is ensemble_pick.EnsemblePicker
    assert commonroad_rp_amd.EnsemblePickResult is ensemble_pick.EnsemblePickResult
    src = _header()
    assert int(re.search(r"#define\s+RP_EPICK_ABI_VERSION\s+(\d+)", src).group(1)) == 1
    # the limits are the ensemble checker's
    ens = open(E.HEADER).read()
    for name in ("MAX_MEMBERS", "MAX_DYN_ROWS", "MAX_POSES", "MAX_VERDICTS"):
        mine = re.search(rf"#define\s+RP_EPICK_{name}\s+(.*)", src).group(1).strip()
        theirs = re.search(rf"#define\s+RP_ENSEMBLE_{name}\s+(.*)", ens).group(1).strip()
        assert mine == theirs, name
        assert getattr(ensemble_pick, name) == getattr(ensemble_check, name)
    assert (ensemble_pick.TRAJ_POSES, ensemble_pick.TRAJ_SWEPT) == (pick.TRAJ_POSES, pick.TRAJ_SWEPT) == (EP.POSES, EP.SWEPT)
    # the struct of the binding is the struct of the header, field by field, as the C compiler lays it out; it starts with rp_pick_result
    names = [n for n, _ in ensemble_pick.RpEpickResult._fields_]
    assert names == RESULT_FIELDS and names[:8] == [n for n, _ in pick.RpPickResult._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rp_epick.h"\nint main(void) {\n  rp_epick_result r = RP_EPICK_RESULT_INIT;\n'
                    '  printf("%u %zu", r.struct_size, sizeof(rp_epick_result));\n' +
                    "".join(f'  printf(" %zu", offsetof(rp_epick_result, {n}));\n' for n in names) +
                    '  printf(" %zu %zu\\n", sizeof(rp_params), sizeof(rp_cost));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(EP.REPO, "include"), "-o", str(exe), str(prog)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = C.sizeof(ensemble_pick.RpEpickResult)
    assert got == [want, want] + [getattr(ensemble_pick.RpEpickResult, n).offset for n in names] + [C.sizeof(_capi.RpParams), C.sizeof(_capi.RpCost)]
    assert want == C.sizeof(pick.RpPickResult) + 16 and ensemble_pick.RpEpickResult().struct_size == want
    for n in names[:8]:
        assert getattr(ensemble_pick.RpEpickResult, n).offset == getattr(pick.RpPickResult, n).offset
    mine = [f.name for f in dataclasses.fields(ensemble_pick.EnsemblePickResult)]
    assert mine == [f.name for f in dataclasses.fields(pick.TrajectoryPickResult)] + ["members_hit", "risk", "best_members_hit", "best_risk"]
    for name in ("set_reference", "set_static", "set_members", "pick", "close", "__enter__", "__exit__"):
        assert callable(getattr(ensemble_pick.EnsemblePicker, name))
    for name in ("label", "reason", "step"):
        assert isinstance(getattr(ensemble_pick.EnsemblePickResult, name), property)


def test_header_compiles_on_its_own(tmp_path):
    body = ("int uses(rp_epick *c, const rp_params *p, const rp_cost *k, rp_epick_result *r) {\n"
            "  return rp_epick_select(c, p, k, RP_TRAJ_POSES | RP_TRAJ_SWEPT, 0.0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, r, 0)\n"
            "         + rp_epick_set_reference(c, 0, 0, 0, 0, 0, 0, 20.0) + rp_epick_set_static(c, 0, 0, 0, 0, 0, 0)\n"
            "         + rp_epick_set_members(c, 1, 0, 0, 0, 0, 0) + (RP_EPICK_MAX_VERDICTS >= ((int64_t)1 << 24) ? 0 : 1) + RP_EPICK_MAX_MEMBERS\n"
            "         + RP_EINVAL + RP_EPICK_ABI_VERSION + RP_N_ARRAYS; }\n")
    others = ('#include "rp_check.h"\n#include "rp_ensemble.h"\n#include "rp_clearance.h"\n#include "rp_score.h"\n#include "rp_lift.h"\n'
              '#include "rp_pick.h"\n#include "rp_amd.h"\n')
    for name, includes in (("only_rp_epick", '#include "rp_epick.h"   /* first and only: the header must be self-contained */\n'),
                           ("epick_then_others", '#include "rp_epick.h"\n' + others), ("others_then_epick", others + '#include "rp_epick.h"\n')):
        src = tmp_path / f"{name}.c"
        src.write_text(includes + body)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(EP.REPO, "include"), "-o", str(tmp_path / f"{name}.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        ensemble_pick.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        ensemble_pick.EnsemblePicker(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        ensemble_pick.EnsemblePicker(0)


def test_makefile_targets_source_hash_inputs_and_capacities():
    src = open(EP.SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "asm" not in re.sub(r"//.*", "", src)
    mk = open(os.path.join(EP.CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1)
    assert "pick" not in srcs and "rules" not in srcs
    assert re.search(r"^EPICKLIB\s*:=\s*\.\./lib/librp_epick\.so$", mk, flags=re.M) and re.search(r"^EPICKDEPS\s*:=.*rp_epick\.hip", mk, flags=re.M)
    assert re.search(r"^all:.*\$\(EPICKLIB\)", mk, flags=re.M) and re.search(r"^epick-resource-usage:", mk, flags=re.M)
    assert re.search(r"^\$\(EPICKLIB\): ", mk, flags=re.M) and re.search(r"^clean:\n\trm -f .*\$\(EPICKLIB\)", mk, flags=re.M)
    # the libraries that include the shared files are rebuilt when these change
    for shared in ("rp_check_rules.h", "rp_lift_rules.h", "rp_lift_walk.inc", "rp_pick_cost.h"):
        assert re.search(rf"^EPICKDEPS\s*:=.* {re.escape(shared)}", mk, flags=re.M), shared
    # the files behind rp_source_hash() and the siblings' own sources define nothing of this library
    for name in srcs.split() + PROTECTED:
        text = open(os.path.join(EP.CSRC, name)).read()
        assert "rp_epick" not in text and not re.search(r"\bEP_", text), name   # (an identifier that starts so: RP_KEEP_... is none)
    # the capacities at which it switches to its device-memory variants are the siblings'
    assert EP.LF_LDS_ROWS == P.LF_LDS_ROWS == L.LDS_ROWS and int(re.search(r"EP_LF_LDS_ROWS\s*=\s*(\d+)", src).group(1)) == L.LDS_ROWS
    assert EP.CK_LDS_ROWS == P.CK_LDS_ROWS == E.LDS_ROWS and int(re.search(r"EP_CK_LDS_ROWS\s*=\s*(\d+)", src).group(1)) == E.LDS_ROWS
    assert EP.MEMBER_BLOCK == int(re.search(r"#else\s*\n\s*constexpr int EP_MEMBER_BLOCK\s*=\s*(\d+);", src).group(1)) >= 1
    # the obstacle walk, the lift step and the cost are stated once: this source takes them from the files that state them
    assert '#include "rp_check_rules.h"' in src and "obb_obb(" not in src and "merge_swept(" not in src
    assert '#include "rp_lift_rules.h"' in src and src.count('#include "rp_lift_walk.inc"') == 1
    assert "rp_sincos(" not in src and "rp_atan(" not in src and "find_segment" not in src
    both = [open(os.path.join(EP.CSRC, name)).read() for name in ("rp_pick.hip", "rp_epick.hip")]
    cost_header = open(os.path.join(EP.CSRC, "rp_pick_cost.h")).read()
    assert "struct PkCost" in cost_header and "desired_speed" in cost_header
    for text in both:
        assert '#include "rp_pick_cost.h"' in text and "struct PkCost" not in text and "50.0 *" not in text
    assert both[0].count('#include "rp_lift_walk.inc"') == 1


# ---- the yardstick: one member is the pick's ---------------------------------------------------------------------------------------
SAME_AS_PICK = ("status", "cost", "best", "best_cost", "n_feasible", "n_collision", "n_collision_before_best", "reason_counts")


def _equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


@pytest.mark.parametrize("name", ["pin"] + list(P.CASES))
def test_reference_with_one_member_is_the_picks_reference(name):
    """One member, NULL weights, max_risk 0: every field equals ``_pick.reference``'s, the lift included"""
    c = EP.single(name)
    want = (P.pin() if name == "pin" else P.case(name)).ref
    got = EP.decide(c.base, None, 0.0)
    assert c.M == 1
    for field in SAME_AS_PICK + ("best_states",):
        assert _equal(getattr(got, field), getattr(want, field)), (name, field)
    assert _equal(got.first_pose_hit[:, 0], want.first_pose_hit) and _equal(got.first_segment_hit[:, 0], want.first_segment_hit), name
    for plane in L.PLANES + ("status", "lengths"):
        assert _equal(getattr(got.lift, plane), getattr(want.lift, plane)), (name, plane)
    hit = (want.first_pose_hit >= 0) | (want.first_segment_hit >= 0)
    assert _equal(got.members_hit, hit.astype(np.int32)) and _equal(got.risk, hit.astype(float)), name
    assert got.best_members_hit == (0 if want.best >= 0 else -1)
    assert got.best_risk == 0.0 if want.best >= 0 else math.isnan(got.best_risk)


@pytest.mark.parametrize("name", list(EP.MULTI) + ["boundary"])
def test_reference_counts_are_the_ensemble_checkers(name):
    """With several members and NULL weights members_hit is ``_ensemble.members_hit`` on the oracle's per-member hits of the feasible
    rows (``_ensemble.oracle_ensemble``: another route to the oracle), and the risk is that count"""
    c = EP.boundary() if name == "boundary" else EP.multi(name)
    b, o = c.base, c.base.lift
    feas = np.flatnonzero(o.status == 1)
    obs = c.obs if c.obs is not None else EP.ObstacleTables()
    lens = o.lengths[feas].astype(np.int32)
    fp, fs = E.oracle_ensemble(c.p, obs, c.members, c.dyn_t0, o.x[feas], o.y[feas], o.theta[feas], lens)
    np.testing.assert_array_equal(b.first_pose_hit[feas], fp if c.mode & EP.POSES else -1)
    np.testing.assert_array_equal(b.first_segment_hit[feas], fs if c.mode & EP.SWEPT else -1)
    count = E.members_hit(fp, fs, bool(c.mode & EP.POSES), bool(c.mode & EP.SWEPT))
    r = EP.decide(b, None, 0.0)
    np.testing.assert_array_equal(r.members_hit[feas], count)
    np.testing.assert_array_equal(r.risk[feas], count.astype(float))
    rest = np.setdiff1d(np.arange(len(o.status)), feas)
    assert (r.members_hit[rest] == 0).all() and (r.risk[rest] == 0.0).all()
    assert (b.first_pose_hit[rest] == -1).all() and (b.first_segment_hit[rest] == -1).all()


# ---- the conditions the GPU tests rest on --------------------------------------------------------------------------------------
def _bounds(c):
    return [float(q) for q in range(c.M + 1)] + [math.inf]


def test_cases_hold_what_the_gpu_tests_rest_on():
    cases = [EP.multi(name) for name in EP.MULTI]
    values, moving, static_total, nan_member = set(), 0, 0, 0
    for c in cases:
        b = c.base
        feas = b.lift.status == 1
        values |= set(int(q) for q in b.members_hit[feas])
        winners = [EP.decide(b, None, bound) for bound in _bounds(c)]
        print(f"{c.name}: M {c.M}, {int(feas.sum())} feasible, members_hit histogram {np.bincount(b.members_hit[feas], minlength=c.M + 1)}, "
              f"winner by bound {[r.best for r in winners]}")
        moving += len(set(r.best for r in winners)) > 1
        # a static hit counts in every member: the trajectory's risk is the total weight
        alone = EP.member_hits(c.p, c.path, E.static_only(c.obs), EP._empty_members(), 0, b.lift, c.mode)
        on_static = np.flatnonzero((alone[0][:, 0] >= 0) | (alone[1][:, 0] >= 0))
        assert (b.members_hit[on_static] == c.M).all()
        w = 0.1 * (1 + np.arange(c.M))
        total = 0.0
        for q in w:
            total = total + float(q)
        assert (EP.decide(b, w, 0.0).risk[on_static] == total).all()
        static_total += len(on_static)
        nan_member += any(np.isnan(c.members[m, :, :, 0]).all(axis=1).any() and not np.isnan(c.members[0, :, :, 0]).all(axis=1).any() for m in range(c.M))
        assert EP.steady(c), c.name
        for r in winners:
            gap = EP.cost_gap(c, r)
            assert gap >= P.COST_GAP or gap == 0.0, (c.name, r.best, gap)
    assert len(values) >= 3 and moving >= 2 and static_total >= 1 and nan_member >= 1
    # the table of the issue this library answers
    c = EP.multi("long_path_m5")
    feas = c.base.lift.status == 1
    assert int(feas.sum()) == 11 and list(np.bincount(c.base.members_hit[feas], minlength=6)) == [4, 1, 0, 2, 0, 4]
    assert [EP.decide(c.base, None, q).best for q in _bounds(c)] == [0, 0, 0, 9, 9, 9, 9]
    c = EP.multi("factor3_m3")
    feas = c.base.lift.status == 1
    assert int(feas.sum()) == 7 and list(np.bincount(c.base.members_hit[feas], minlength=4)) == [3, 2, 2, 0]
    assert [EP.decide(c.base, None, q).best for q in _bounds(c)] == [6, 6, 2, 2, 2]
    assert EP.multi("long_path_m65").M == 65 and EP.multi("long_path_m65").planes[0].shape == (16, 31)
    assert len(EP.multi("long_path_m5").path.pos) - 1 == EP.LF_LDS_ROWS + 1


def test_boundary_case_holds_what_its_name_says():
    c = EP.boundary()
    B, n = EP.BOUNDARY_BLOCK, EP.BOUNDARY_N
    assert c.M == 2 * B and c.planes[0].shape == (4, n) and n > 64 and c.p.factor == 3 and c.mode == EP.POSES | EP.SWEPT
    fp, fs = np.full((4, c.M), -1, np.int32), np.full((4, c.M), -1, np.int32)
    for k, m, i, kind in EP.boundary_plan():
        (fp if kind == "pose" else fs)[k, m] = i
        if kind == "segment":   # the rectangle's time index time_step0 + i is segment i's, and no pose's (time_step0 + j * factor)
            assert i % int(c.p.factor) != 0
    np.testing.assert_array_equal(c.base.first_pose_hit, fp)
    np.testing.assert_array_equal(c.base.first_segment_hit, fs)
    assert {63, 64} <= set(fp[0]) and fp[0, 0] >= 0 and fp[0, B - 1] >= 0 and fp[0, B] >= 0 and fp[0, 2 * B - 1] >= 0
    np.testing.assert_array_equal(c.base.lift.status[:3], 1)
    assert c.base.lift.status[3] != 1 and EP.steady(c)
    r = EP.decide(c.base, None, 0.0)
    assert r.status[0] == EP.S.status_word(3, 0, 63) and r.status[1] == EP.S.status_word(3, 0, 62) and r.best == 2


# ---- the order of the risk -------------------------------------------------------------------------------------------------------
def test_risk_is_the_ascending_sum_and_the_order_shows():
    c = EP.multi("long_path_m5")
    w = 0.1 * (1 + np.arange(c.M))   # 0.1, 0.2, 0.3, ...
    r = EP.decide(c.base, w, 0.0)
    up, down = np.zeros(len(r.risk)), np.zeros(len(r.risk))
    for k in range(len(r.risk)):
        for m in range(c.M):
            if c.base.hit[k, m]:
                up[k] = up[k] + w[m]
        for m in reversed(range(c.M)):
            if c.base.hit[k, m]:
                down[k] = down[k] + w[m]
    np.testing.assert_array_equal(r.risk.view(np.uint64), up.view(np.uint64))
    assert (up != down).any() and np.allclose(up, down, rtol=1e-15, atol=0)
    # with unit weights the risk is the count, exactly; a weight of zero counts in members_hit and not in the risk
    np.testing.assert_array_equal(EP.decide(c.base, None, 0.0).risk, c.base.members_hit.astype(float))
    z = np.ones(c.M)
    z[0] = 0.0
    rz = EP.decide(c.base, z, 0.0)
    np.testing.assert_array_equal(rz.members_hit, c.base.members_hit)
    np.testing.assert_array_equal(rz.risk, c.base.hit[:, 1:].sum(axis=1).astype(float))
    assert (rz.risk < rz.members_hit).any()
