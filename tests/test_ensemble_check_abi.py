"""librp_ensemble.so exports what include/rp_ensemble.h declares and what the binding of commonroad_rp_amd.ensemble_check binds -- no
more, no less; nothing of it went into the other two libraries; the header stands on its own; without the library or without a GPU an
ensemble checker fails loudly.  No compute calls here (the GPU tests are in tests/test_ensemble_check.py)."""
import os
import re
import subprocess

import pytest

import commonroad_rp_amd
from commonroad_rp_amd import _capi, ensemble_check, trajectory_check

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rp_ensemble.h")
SOURCE = os.path.join(REPO, "commonroad-reactive-planner_amd", "csrc", "rp_ensemble.hip")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared_functions():
    return sorted(set(re.findall(r"\b(rp_[a-z_]+)\s*\(", _header())))


def _library():
    if not all(os.path.exists(p) for p in (ensemble_check.LIB_PATH, trajectory_check.LIB_PATH, _capi.LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return ensemble_check.LIB_PATH


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("rp_") and ln.split()[-2] in "TW")


def test_header_binding_and_library_agree():
    declared = _declared_functions()
    assert declared == sorted(ensemble_check.EXPORTED_SYMBOLS)
    assert len(declared) == 7 and all(name.startswith("rp_ensemble_") for name in declared)
    assert not any(ch.isdigit() for name in declared for ch in name)
    assert _exported(_library()) == declared


def test_the_other_two_libraries_are_what_they_were():
    _library()
    planning, checker = _exported(_capi.LIB_PATH), _exported(trajectory_check.LIB_PATH)
    assert planning and not any(name.startswith(("rp_checker", "rp_ensemble")) for name in planning)
    assert checker == sorted(trajectory_check.EXPORTED_SYMBOLS) and all(name.startswith("rp_checker_") for name in checker)
    assert not any(name.startswith(("rp_checker", "rp_ensemble")) for name in _capi.EXPORTED_SYMBOLS)
    assert not any(name.startswith("rp_ensemble") for name in trajectory_check.EXPORTED_SYMBOLS)


def test_abi_version_limits_and_package_exports():
    lib = ensemble_check.load_library(_library())
    assert lib.rp_ensemble_abi_version() == ensemble_check.ABI_VERSION == 1
    assert commonroad_rp_amd.EnsembleChecker is ensemble_check.EnsembleChecker
    assert commonroad_rp_amd.EnsembleCheckResult is ensemble_check.EnsembleCheckResult
    assert commonroad_rp_amd.TrajectoryChecker is trajectory_check.TrajectoryChecker   # (beside the two already there)
    src = _header()
    assert int(re.search(r"#define\s+RP_ENSEMBLE_ABI_VERSION\s+(\d+)", src).group(1)) == 1
    assert int(re.search(r"#define\s+RP_ENSEMBLE_MAX_MEMBERS\s+(\d+)", src).group(1)) == ensemble_check.MAX_MEMBERS == 4096
    for name, value, want in (("RP_ENSEMBLE_MAX_DYN_ROWS", ensemble_check.MAX_DYN_ROWS, 1 << 22),
                              ("RP_ENSEMBLE_MAX_POSES", ensemble_check.MAX_POSES, 1 << 24),
                              ("RP_ENSEMBLE_MAX_VERDICTS", ensemble_check.MAX_VERDICTS, 1 << 24)):
        assert 1 << int(re.search(rf"#define\s+{name}\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", src).group(1)) == value == want
    assert (ensemble_check.TRAJ_POSES, ensemble_check.TRAJ_SWEPT) == (trajectory_check.TRAJ_POSES, trajectory_check.TRAJ_SWEPT) == tuple(
        int(re.search(rf"#define\s+{n}\s+(\d+)u", src).group(1)) for n in ("RP_TRAJ_POSES", "RP_TRAJ_SWEPT"))


def test_header_compiles_on_its_own_and_beside_the_checker_header(tmp_path):
    body = ("int uses(rp_ensemble *e, const rp_params *p, int32_t *members_hit, int64_t *ff, int64_t *no) {\n"
            "  return rp_ensemble_check(e, p, RP_TRAJ_POSES | RP_TRAJ_SWEPT, 0, 1, 0, 0, 0, 0, 0, 0, 0, members_hit, ff, no)\n"
            "         + rp_ensemble_set_members(e, RP_ENSEMBLE_MAX_MEMBERS, 0, 0, 0, 0) + rp_ensemble_set_static(e, 0, 0, 0, 0, 0, 0)\n"
            "         + (RP_ENSEMBLE_MAX_POSES >= RP_ENSEMBLE_MAX_VERDICTS && RP_ENSEMBLE_MAX_DYN_ROWS > 0 ? 0 : 1) + RP_EINVAL; }\n")
    for name, includes in (("only_rp_ensemble", '#include "rp_ensemble.h"   /* first and only: the header must be self-contained */\n'),
                           ("ensemble_then_check", '#include "rp_ensemble.h"\n#include "rp_check.h"\n'),
                           ("check_then_ensemble", '#include "rp_check.h"\n#include "rp_ensemble.h"\n')):
        src = tmp_path / f"{name}.c"
        src.write_text(includes + body)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / f"{name}.o"), str(src)])


def test_missing_library_fails_loudly(tmp_path):
    missing = str(tmp_path / "nope.so")
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        ensemble_check.load_library(missing)
    with pytest.raises(_capi.RpLibraryMissing, match="nope.so"):
        ensemble_check.EnsembleChecker(0, library=missing)


def test_create_without_gpu_reports_error_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _library()
    with pytest.raises(_capi.RpError):
        ensemble_check.EnsembleChecker(0)


def test_no_environment_reads_no_prints_and_no_inline_assembly():
    src = open(SOURCE).read()
    assert "getenv" not in src
    assert "printf" not in src and "assert(" not in src.replace("static_assert(", "")
    assert "asm" not in re.sub(r"//.*", "", src)


def test_member_block_and_lds_capacity_are_readable_from_the_source():
    """tests/_ensemble.py sizes its cases by them: a case list built on the fallbacks would miss the kernel's thresholds."""
    import _ensemble
    src = open(SOURCE).read()
    assert _ensemble.MEMBER_BLOCK == int(re.search(r"\bEN_MEMBER_BLOCK\s*=\s*(\d+)\s*;", src).group(1)) >= 1
    assert _ensemble.LDS_ROWS == int(re.search(r"\bEN_LDS_ROWS\s*=\s*(\d+)\s*;", src).group(1))
    Ms = [c[-1] for c in _ensemble.CASES[-3:]]
    assert Ms == ([_ensemble.MEMBER_BLOCK + d for d in (-1, 0, 1)] if _ensemble.MEMBER_BLOCK > 1 else [1, 2, 3])
