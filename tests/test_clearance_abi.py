"""librp_clearance.so exports what include/rp_clearance.h declares and what the binding of commonroad_rp_amd.clearance binds -- no
more, no less; the header stands on its own; without the library or without a GPU a ClearanceQuery fails loudly.  Then, on the CPU
alone, the NumPy reference of tests/_clearance.py: known answers, and the conditions the GPU tests of tests/test_clearance.py rest
on.  No compute calls on the device here."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, clearance, ensemble_check, trajectory_check

import _clearance as R
from test_trajectory_check import _oracle_tables

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = R.HEADER
SOURCE = R.SOURCE


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared_functions():
    return sorted(set(re.findall(r"\b(rp_[a-z_]+)\s*\(", _header())))


def _library():
    if not all(os.path.exists(p) for p in (clearance.LIB_PATH, trajectory_check.LIB_PATH, _capi.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return clearance.LIB_PATH


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")


def test_header_binding_and_library_agree():
    declared = _declared_functions()
    assert declared == sorted(clearance.EXPORTED_SYMBOLS)
    assert len(declared) == 6 and all(name.startswith("rp_clearance_") for name in declared)
    assert not any(ch.isdigit() for name in declared for ch in name)
    assert _exported(_library()) == declared
    # the other libraries' tables are what they were: nothing of the clearance query went into them
    for other in (_capi.EXPORTED_SYMBOLS, trajectory_check.EXPORTED_SYMBOLS, ensemble_check.EXPORTED_SYMBOLS):
        assert not any(name.startswith("rp_clearance") for name in other)
    assert not any(name.startswith("rp_clearance") for name in _exported(_capi.LIB_PATH) + _exported(trajectory_check.LIB_PATH))


def test_abi_version_limits_and_package_exports():
    lib = clearance.load_library(_library())
    assert lib.rp_clearance_abi_version() == clearance.ABI_VERSION == 1
    assert commonroad_rp_amd.ClearanceQuery is clearance.ClearanceQuery
    assert commonroad_rp_amd.ClearanceResult is clearance.ClearanceResult
    src = _header()
    assert int(re.search(r"#define\s+RP_CLEARANCE_ABI_VERSION\s+(\d+)", src).group(1)) == 1
    assert int(re.search(r"#define\s+RP_CLEARANCE_MAX_POSES\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", src).group(1)) == 24
    assert clearance.MAX_POSES == 1 << 24
    tiny = float(re.search(r"#define\s+RP_CLEARANCE_TINY\s+(\S+)", src).group(1))
    assert tiny == clearance.TINY == np.finfo(np.float64).tiny and tiny > 0.0
    assert [f.name for f in __import__("dataclasses").fields(clearance.ClearanceResult)] == [
        "pose_clearance", "min_clearance", "min_pose", "nearest", "first_clear", "n_below", "best"]


def test_header_compiles_on_its_own(tmp_path):
    body = ("int uses(rp_clearance *c, const rp_params *p, int64_t *fc, int64_t *nb, int64_t *best) {\n"
            "  return rp_clearance_query(c, p, 0, 1, 0, 0, 0, 0, 5.0, 0.0, 0, 0, 0, 0, fc, nb, best)\n"
            "         + (RP_CLEARANCE_MAX_POSES >= ((int64_t)1 << 24) ? 0 : 1) + (RP_CLEARANCE_TINY > 0.0 ? 0 : 1) + RP_EINVAL; }\n")
    for name, includes in (("only_rp_clearance", '#include "rp_clearance.h"   /* first and only: the header must be self-contained */\n'),
                           ("clearance_then_check", '#include "rp_clearance.h"\n#include "rp_check.h"\n#include "rp_ensemble.h"\n'),
                           ("check_then_clearance", '#include "rp_check.h"\n#include "rp_ensemble.h"\n#include "rp_clearance.h"\n')):
        src = tmp_path / f"{name}.c"
        src.write_text(includes + body)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / f"{name}.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        clearance.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        clearance.ClearanceQuery(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        clearance.ClearanceQuery(0)


def test_no_environment_reads_and_no_inline_assembly():
    src = open(SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "asm" not in re.sub(r"//.*", "", src)
    # the files that enter rp_source_hash() are only included, and nothing of the new library enters SRCS
    mk = open(os.path.join(os.path.dirname(SOURCE), "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1)
    assert "clearance" not in srcs
    assert re.search(r"^all:.*\$\(CLRLIB\)", mk, flags=re.M) and re.search(r"^clearance-resource-usage:", mk, flags=re.M)
    assert re.search(r"^\$\(CLRLIB\): rp_clearance\.hip ", mk, flags=re.M)


# ---- the reference: known answers --------------------------------------------------------------------------------------------
def _rect(cx, cy, th, hl, hw):
    return R.rect_polygon(cx, cy, th, hl, hw)[None]


def test_reference_known_answers():
    unit = _rect(0.0, 0.0, 0.0, 1.0, 0.5)                                    # [-1, 1] x [-0.5, 0.5]
    # axis-aligned rectangles 3 m apart, along x and along y
    assert R.polygon_distance(unit, _rect(6.0, 0.2, 0.0, 2.0, 2.0))[0] == pytest.approx(3.0, abs=1e-12)
    assert R.polygon_distance(unit, _rect(0.3, -4.5, 0.0, 0.2, 1.0))[0] == pytest.approx(3.0, abs=1e-12)
    # corner to corner: (1, 0.5) to (4, 4.5) is 5
    assert R.polygon_distance(unit, _rect(5.0, 5.5, 0.0, 1.0, 1.0))[0] == pytest.approx(5.0, abs=1e-12)
    # corner to edge at 45 degrees: a square of half side 1 turned by 45 degrees has a corner at distance sqrt(2) from its centre; with
    # the centre at (4, 0) that corner is at x = 4 - sqrt(2), the unit rectangle's edge at x = 1
    assert R.polygon_distance(unit, _rect(4.0, 0.0, math.pi / 4, 1.0, 1.0))[0] == pytest.approx(3.0 - math.sqrt(2.0), abs=1e-12)
    # ... and the other way round: an EDGE of a turned square (half side 3) on the line x + y = 3, its midpoint (1.75, 1.25) the foot
    # of the corner (1, 0.5): (3 - 1.5) / sqrt(2)
    sq = _rect(1.75 + 3.0 / math.sqrt(2.0), 1.25 + 3.0 / math.sqrt(2.0), math.pi / 4, 3.0, 3.0)
    assert R.polygon_distance(unit, sq)[0] == pytest.approx(1.5 / math.sqrt(2.0), abs=1e-12)
    # touching and overlapping and containment: 0, both ways
    assert R.polygon_distance(unit, _rect(2.0, 0.0, 0.0, 1.0, 0.5))[0] == 0.0
    assert R.polygon_distance(unit, _rect(0.5, 0.2, 0.3, 1.0, 0.5))[0] == 0.0
    assert R.polygon_distance(unit, _rect(0.1, 0.1, 1.0, 0.05, 0.05))[0] == 0.0
    assert R.polygon_distance(_rect(0.1, 0.1, 1.0, 0.05, 0.05), unit)[0] == 0.0
    assert R.polygon_distance(unit, _rect(0.0, 0.0, 0.5, 10.0, 10.0))[0] == 0.0
    # a cross: no vertex of either inside the other, still 0
    assert R.polygon_distance(_rect(0.0, 0.0, 0.0, 3.0, 0.2), _rect(0.0, 0.0, math.pi / 2, 3.0, 0.2))[0] == 0.0
    # triangles: a vertex facing the rectangle's edge, an edge facing the rectangle's corner, containment
    tri = np.array([[[3.0, 0.0], [5.0, -1.0], [5.0, 1.0]]])
    assert R.polygon_distance(unit, tri)[0] == pytest.approx(2.0, abs=1e-12)
    tri = np.array([[[3.0, 0.5], [1.0, 2.5], [4.0, 4.0]]])                    # its edge (3, 0.5)-(1, 2.5) lies on x + y = 3.5
    assert R.polygon_distance(unit, tri)[0] == pytest.approx((3.5 - 1.5) / math.sqrt(2.0), abs=1e-12)
    assert R.polygon_distance(unit, np.array([[[-9.0, -9.0], [9.0, -9.0], [0.0, 9.0]]]))[0] == 0.0
    assert R.polygon_distance(unit, np.array([[[0.0, 0.0], [0.2, 0.0], [0.0, 0.2]]]))[0] == 0.0
    # circles: beside an edge, off a corner, overlapping, centre inside, rectangle inside the disc
    assert R.circle_distance(unit, 4.0, 0.1, 1.0)[0] == pytest.approx(2.0, abs=1e-12)
    assert R.circle_distance(unit, 4.0, 4.5, 1.5)[0] == pytest.approx(3.5, abs=1e-12)
    assert R.circle_distance(unit, 1.5, 0.0, 0.5)[0] == 0.0
    assert R.circle_distance(unit, 0.3, 0.1, 0.01)[0] == 0.0
    assert R.circle_distance(unit, 0.0, 0.0, 50.0)[0] == 0.0


def test_reference_table_rules():
    """Ids follow static rectangles, triangles, circles, dynamic obstacles; a dynamic obstacle counts at time index time_step0 + i *
    factor only, a NaN row and an index outside the table mean absent; poses behind the end see nothing."""
    from commonroad_rp_amd.collision import ObstacleTables
    n = 6
    x, y, th = 10.0 * np.arange(n)[None, :], np.zeros((1, n)), np.zeros((1, n))
    dyn = np.full((2, 4, 5), np.nan)
    dyn[0, 1] = (x[0, 1] + R.WB, 5.0, 0.0, 1.0, 1.0)          # table index 1 = time index 3 = pose 1 with factor 1, time_step0 2
    dyn[1, 3] = (x[0, 1] + R.WB, 0.0, 0.0, 1.0, 1.0)          # time index 5 = pose 3 (factor 1) or pose 1 (factor 3)
    obs = ObstacleTables(static_obb=[[0.0, 40.0, 0.0, 1.0, 1.0]], static_tri=[[0, -40, 1, -40, 0, -41]], static_circ=[[20.0 + R.WB, 0.0, 0.5]],
                         dyn_obb=dyn, dyn_t0=2)
    p = R._params(time_step0=2, factor=1, n=n)
    D = R.reference(p, obs, x, y, th, lengths=[5])
    assert D.shape == (1, n, 5)
    assert np.isinf(D[0, 5]).all() and np.isfinite(D[0, :5, :3]).all()
    assert D[0, 2, 2] == 0.0                                   # the disc sits on pose 2
    assert D[0, 1, 3] == pytest.approx(5.0 - 1.0 - R.HW, abs=1e-12) and np.isinf(np.delete(D[0, :, 3], 1)).all()
    assert np.isinf(D[0, :, 4]).sum() == n - 1 and D[0, 3, 4] == pytest.approx(20.0 - R.HL - 1.0, abs=1e-12)
    D3 = R.reference(R._params(time_step0=2, factor=3, n=n), obs, x, y, th)
    assert D3[0, 1, 4] == 0.0 and np.isinf(np.delete(D3[0, :, 4], 1)).all() and np.isinf(D3[0, :, 3]).all()
    clear, near = R.nearest_of(D)
    assert near[0, 2] == 2 and clear[0, 2] == 0.0 and near[0, 5] == -1 and np.isinf(clear[0, 5])
    clear, near = R.nearest_of(D, cutoff=1.0)
    assert (near[0] == [-1, -1, 2, -1, -1, -1]).all() and np.isinf(np.delete(clear[0], 2)).all()


# ---- the conditions the GPU tests rest on --------------------------------------------------------------------------------------
def test_reference_zero_is_the_oracle_hit_on_every_pose():
    """(a) reference zero <=> oracle.check_poses hit, on every pose of every case; (d) both outcomes occur."""
    from oracle import oracle
    poses = hits = mismatches = 0
    for c in R.cases():
        tb = _oracle_tables(c.obs)
        for k in range(c.x.shape[0]):
            L = c.x.shape[1] if c.lengths is None else int(c.lengths[k])
            h, _ = oracle.check_poses(c.p, tb, c.x[k, :L], c.y[k, :L], c.th[k, :L])
            zero = c.clear[k, :L] == 0.0
            poses, hits, mismatches = poses + L, hits + int(h.sum()), mismatches + int((zero != h).sum())
            assert np.isinf(c.clear[k, L:]).all()
    print(f"poses {poses} hits {hits} mismatches {mismatches}")
    assert mismatches == 0
    assert poses == sum(int(c.valid.sum()) for c in R.cases())   # no pose left out
    assert 20 * hits >= poses and 5 * (poses - hits) >= poses, (hits, poses)


def test_reference_distances_keep_clear_of_zero_the_cutoff_and_the_margin():
    """(b) no reference distance in (0, 1e-6); (c) none within 1e-6 of the cutoff or the margin the GPU tests use; the cutoff lies
    inside the range of clearances that occur; every kind of obstacle is the nearest one somewhere."""
    smallest = math.inf
    below = above = 0
    for c in R.cases():
        D = c.D[np.isfinite(c.D)]
        pos = D[D > 0.0]
        if pos.size:
            smallest = min(smallest, float(pos.min()))
        for level in (R.CUTOFF, R.MARGIN):
            assert not (np.abs(D - level) <= 1e-6).any(), level
        fin = c.clear[np.isfinite(c.clear)]
        below, above = below + int((fin <= R.CUTOFF).sum()), above + int((fin > R.CUTOFF).sum())
        mins = c.clear.min(axis=1)
        assert not (np.abs(mins[np.isfinite(mins)] - R.MARGIN) <= 1e-6).any()
    print(f"smallest positive reference distance {smallest:.3e}; clearances <= cutoff {below}, above {above}")
    assert smallest >= 1e-6
    assert below >= 100 and above >= 100
    big = R.cases()[R.DEVICE_MEMORY_CASE]
    ns, nt = len(big.obs.static_obb), len(big.obs.static_tri)
    kinds = {("obb" if i < ns else "tri" if i < ns + nt else "circ" if i < R.n_static_of(big.obs) else "dyn") for i in big.near[big.near >= 0]}
    assert kinds == {"obb", "tri", "circ", "dyn"}
    # ... and in that case (factor 3, the kernel variant that reads the static rows from device memory) positive clearances hang on
    # the dynamic table
    assert ((big.near >= R.n_static_of(big.obs)) & (big.clear > 0.0)).sum() >= 5
    assert R.n_static_of(big.obs) == R.LDS_ROWS + 1
