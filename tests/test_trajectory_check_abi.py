"""librp_check.so exports what include/rp_check.h declares and what the binding of commonroad_rp_amd.trajectory_check
binds -- no more, no less; the header stands on its own; without the library or without a GPU a checker fails loudly.
No compute calls here (the GPU tests are in tests/test_trajectory_check.py)."""
import os
import re
import subprocess

import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, trajectory_check

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rp_check.h")
SOURCE = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_check.hip")


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rp_[a-z_]+)\s*\(", src)))


def _library():
    if not os.path.exists(trajectory_check.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return trajectory_check.LIB_PATH


def test_header_binding_and_library_agree():
    declared = _declared_functions()
    assert declared == sorted(trajectory_check.EXPORTED_SYMBOLS)
    assert len(declared) == 6 and all(name.startswith("rp_checker_") for name in declared)
    assert not any(ch.isdigit() for name in declared for ch in name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _library()]).decode()
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")
    assert exported == declared
    # the planning library's table is what it was: nothing of the checker went into it
    assert not any(name.startswith("rp_checker") for name in _capi.EXPORTED_SYMBOLS)


def test_abi_version_and_package_exports():
    lib = trajectory_check.load_library(_library())
    assert lib.rp_checker_abi_version() == trajectory_check.ABI_VERSION == 1
    assert commonroad_rp_amd.TrajectoryChecker is trajectory_check.TrajectoryChecker
    assert commonroad_rp_amd.TrajectoryCheckResult is trajectory_check.TrajectoryCheckResult
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+RP_CHECKER_MAX_POSES\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", src).group(1)) >= 24
    assert trajectory_check.MAX_POSES == 1 << 24
    assert (trajectory_check.TRAJ_POSES, trajectory_check.TRAJ_SWEPT) == tuple(
        int(re.search(rf"#define\s+{n}\s+(\d+)u", src).group(1)) for n in ("RP_TRAJ_POSES", "RP_TRAJ_SWEPT"))


def test_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "only_rp_check.c"
    src.write_text('#include "rp_check.h"   /* first and only: the header must be self-contained */\n'
                   "int uses(rp_checker *c, const rp_params *p, int64_t *ff, int64_t *nh) {\n"
                   "  return rp_checker_check(c, p, RP_TRAJ_POSES | RP_TRAJ_SWEPT, 0, 1, 0, 0, 0, 0, 0, 0, 0, ff, nh)\n"
                   "         + (RP_CHECKER_MAX_POSES >= ((int64_t)1 << 24) ? 0 : 1) + RP_EINVAL; }\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "only_rp_check.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        trajectory_check.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        trajectory_check.TrajectoryChecker(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        trajectory_check.TrajectoryChecker(0)


def test_no_environment_reads_and_no_inline_assembly():
    src = open(SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "asm" not in re.sub(r"//.*", "", src)
