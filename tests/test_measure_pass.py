"""``profiles/measure.py``, the driver of a round's measurement pass, without a GPU: its counter summaries against what the scripts
it replaced computed on the same CSVs (``tests/golden/counters_small/``), its step runner's fail-stop on harmless children, the
all-or-nothing install of records, and the plan of a whole pass (``all --dry-run``)."""
import json
import os
import shlex
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "profiles"))
import measure   # noqa: E402

SMALL = os.path.join(REPO, "tests", "golden", "counters_small")
PY = sys.executable
FAULT = "an illegal memory access was encountered"


# ------------------------------------------------------------------------------------------ summaries against the parent's scripts
# tests/golden/counters_small/: the first five launches per kernel of one pass's cfg2 counter CSVs (four columns kept), plus rows
# written by hand: a costs-only instance of rp_eval_kernel on the same grid with MORE launches than the state-writing one and far
# less written, three one-workgroup launches of the state-writing instance with absurd values (not the largest grid: to be left
# out), and rp_lon_kernel on two grids.  The expected entries are what pmc_summary.py, fp64_summary.py and sq_summary.py of the
# commit before this driver printed for these directories.

WRITING = "void rp_eval_kernel<16, true, false, 1, false, false, true, 256, false>"
COSTS_ONLY = "void rp_eval_kernel<16, false, false, 1, false, false, true, 256, false>"
BENCH_LINE = os.path.join(SMALL, "bench.json")


def test_traffic_entry_is_what_pmc_summary_computed():
    # (the instance with the largest median WRITE_SIZE, not the one with the most launches; its launches of the largest grid only --
    # with the three small ones the median would be 18505.3125 KB; FETCH_SIZE doubled: 598.9375 KB x 1024 x 2)
    assert measure.traffic_entry(os.path.join(SMALL, "traffic"), "cfg2", "draw", BENCH_LINE) == {
        "workload": "cfg2", "mode": "draw", "kernel": WRITING, "write_bytes": 18920768.0, "fetch_bytes_corrected_x2": 1226624.0,
        "traffic_bytes": 20147392.0,
        "detail": {"WRITE_SIZE": {"kernel": WRITING, "median_KB": 18477.3125, "n": 5}, "FETCH_SIZE": {"kernel": WRITING, "median_KB": 598.9375, "n": 5}},
        "other_kernels": {"rp_finalize_kernel": {"write_bytes": 7904.0, "launches": 5, "fetch_bytes": 49408.0},
                          "void rp_lon_kernel<16, false, true>": {"write_bytes": 655872.0, "launches": 3, "fetch_bytes": 68608.0}}}


def test_fp64_entry_is_what_fp64_summary_computed():
    # (read from the instance with the most launches of the largest grid; flops = 64 x (ADD + MUL + TRANS + 2 FMA))
    assert measure.fp64_entry(os.path.join(SMALL, "fp64"), "cfg2", "fused", BENCH_LINE) == {
        "workload": "cfg2", "mode": "fused", "kernel": COSTS_ONLY, "candidates": 7440.0, "steps": 31,
        "wave_instructions": {"ADD": 61003.0, "MUL": 150003.0, "FMA": 170003.0, "TRANS": 9003.0}, "waves": 1863.0,
        "flops_per_launch": 35840960.0, "flops_per_candidate_step": 155.3978494623656,
        "model": "64 lanes x (ADD_F64 + MUL_F64 + TRANS_F64 + 2 FMA_F64) wavefront instructions counted by the SQ block (rocprofv3 --pmc), "
                 "median launch, / (candidates x (N + 1))"}
    assert 35840960.0 == 64.0 * (61003.0 + 150003.0 + 9003.0 + 2.0 * 170003.0)


def test_sq_kernels_are_what_sq_summary_computed():
    # (sq/: three launches per rp_eval_kernel instance, one per other kernel, of the same pass's two cfg3 SQ counter groups -- among them
    # rp_chunk_kernel, which the bench line's kernel family leaves out, and one-workgroup launches of another rp_eval_kernel instance)
    sq = os.path.join(SMALL, "sq")
    assert measure.sq_kernels(sq, os.path.join(sq, "bench.json")) == {
        "void rp_eval_kernel<16, false, false, 2, false, false, false, 256, false>": {
            "SQ_INSTS_LDS": 1117008.0, "SQ_INSTS_SALU": 13924693.0, "SQ_INSTS_SMEM": 1270939.0, "SQ_INSTS_VALU": 30855342.0,
            "SQ_INSTS_VMEM_RD": 1571689.0, "SQ_INSTS_VMEM_WR": 89838.0, "SQ_WAVES": 15624.0, "SQ_ACTIVE_INST_ANY": 53424963.0,
            "SQ_ACTIVE_INST_SCA": 15195632.0, "SQ_ACTIVE_INST_VALU": 31241016.0, "SQ_BUSY_CYCLES": 6970060.0, "SQ_INST_CYCLES_SALU": 13924693.0,
            "SQ_WAIT_INST_ANY": 25735684.0, "SQ_WAVE_CYCLES": 145209102.0,
            "per_wave": {"SQ_INSTS_LDS": 71.5, "SQ_INSTS_SALU": 891.2, "SQ_INSTS_SMEM": 81.3, "SQ_INSTS_VALU": 1974.9, "SQ_INSTS_VMEM_RD": 100.6, "SQ_INSTS_VMEM_WR": 5.8}},
        "void rp_eval_kernel<16, true, false, 2, false, false, false, 256, false>": {
            "SQ_INSTS_LDS": 1207038.0, "SQ_INSTS_SALU": 14907544.0, "SQ_INSTS_SMEM": 1930771.0, "SQ_INSTS_VALU": 31410419.0,
            "SQ_INSTS_VMEM_RD": 1504005.0, "SQ_INSTS_VMEM_WR": 933534.0, "SQ_WAVES": 15624.0, "SQ_ACTIVE_INST_ANY": 57031545.0,
            "SQ_ACTIVE_INST_SCA": 16838315.0, "SQ_ACTIVE_INST_VALU": 31811810.0, "SQ_BUSY_CYCLES": 7650427.0, "SQ_INST_CYCLES_SALU": 14907544.0,
            "SQ_WAIT_INST_ANY": 31857506.0, "SQ_WAVE_CYCLES": 160399035.0,
            "per_wave": {"SQ_INSTS_LDS": 77.3, "SQ_INSTS_SALU": 954.1, "SQ_INSTS_SMEM": 123.6, "SQ_INSTS_VALU": 2010.4, "SQ_INSTS_VMEM_RD": 96.3, "SQ_INSTS_VMEM_WR": 59.8}},
    }


# ------------------------------------------------------------------------------------------------------------------ fail-stop

def _three_steps(second):
    """a stage of three steps whose second runs the Python source ``second``; its one record would replace r05_sq_cfg3.json"""
    def stage(run):
        run.step("first", "quick", [PY, "-c", "print('first')"])
        run.step("second", "quick", [PY, "-c", second])
        run.step("third", "quick", [PY, "-c", "print('third')"])
        return {"r05_sq_cfg3.json": json.dumps({"source_hash": "aaaa"})}
    return stage


@pytest.fixture
def pass_dirs(tmp_path, monkeypatch):
    """(runner on an output directory, a directory standing in for profiles/ with one installed record)"""
    monkeypatch.setitem(measure.LIMITS, "quick", 1)
    dest = tmp_path / "profiles"
    dest.mkdir()
    (dest / "r05_sq_cfg3.json").write_text("as found")
    return measure.Runner(str(tmp_path / "out")), dest


def _steps(run):
    return [json.loads(l) for l in open(os.path.join(run.out, "steps.jsonl"))]


@pytest.mark.parametrize("second, status", [("import sys; sys.exit(3)", 3), ("import sys; sys.exit(134)", 134),
                                            ("import time; time.sleep(5)", 124)])
def test_nothing_is_started_or_installed_after_a_failed_step(pass_dirs, capsys, second, status):
    run, dest = pass_dirs
    assert measure.run_stage(_three_steps(second), run, "aaaa", str(dest)) != 0
    steps = _steps(run)
    assert [s["step"] for s in steps] == ["first", "second"] and not os.path.exists(os.path.join(run.out, "third.out"))
    assert [s["status"] for s in steps] == [0, status]
    assert steps[1]["argv"][:4] == ["timeout", "-k", "10", "1"] and steps[1]["limit"] == 1 and steps[1]["seconds"] < 4
    assert os.listdir(str(dest)) == ["r05_sq_cfg3.json"] and (dest / "r05_sq_cfg3.json").read_text() == "as found"
    said = capsys.readouterr().err
    assert "second" in said and f"status {status}" in said and os.path.join(run.out, "second.err") in said


def test_a_reported_gpu_fault_fails_a_step_that_exits_0(pass_dirs, capsys):
    run, dest = pass_dirs
    assert measure.run_stage(_three_steps(f"print('HIP error: {FAULT}')"), run, "aaaa", str(dest)) != 0
    assert [(s["step"], s["status"]) for s in _steps(run)] == [("first", 0), ("second", 0)]
    assert (dest / "r05_sq_cfg3.json").read_text() == "as found"
    assert os.path.join(run.out, "second.out") in capsys.readouterr().err


def test_a_stage_whose_steps_all_succeed_installs_its_records(pass_dirs):
    run, dest = pass_dirs
    assert measure.run_stage(_three_steps("print('second')"), run, "aaaa", str(dest)) == 0
    assert [(s["step"], s["status"]) for s in _steps(run)] == [("first", 0), ("second", 0), ("third", 0)]
    assert json.loads((dest / "r05_sq_cfg3.json").read_text()) == {"source_hash": "aaaa"}
    assert os.listdir(str(dest)) == ["r05_sq_cfg3.json"]                        # (no temporary file left beside it)
    assert open(os.path.join(run.out, "second.out")).read() == "second\n"


# ----------------------------------------------------------------------------------------------------- all-or-nothing install

def _parity(h):
    return f"Fuzz sweeps (tests/sweeps/fuzz_parity.py) on MI355X, library source hash {h}\ndefault launch paths, seeds 1 .. 2:\n"


def test_records_of_two_libraries_or_of_another_library_are_refused(tmp_path):
    dest = str(tmp_path)
    sq = lambda h: json.dumps({"workload": "cfg3", "source_hash": h, "kernels": {}})
    with pytest.raises(measure.Refused):   # two hashes among the records of one stage
        measure.install({"r05_sq_cfg3.json": sq("aaaa"), "r05_sq_cfg5_fused.json": sq("bbbb")}, "aaaa", dest)
    with pytest.raises(measure.Refused):   # one hash, not the loaded library's
        measure.install({"r05_sq_cfg3.json": sq("bbbb"), "r05_sq_cfg5_fused.json": sq("bbbb")}, "aaaa", dest)
    with pytest.raises(measure.Refused):
        measure.install({"r05_fuzz_parity.txt": _parity("aaaa"), "r05_full_scale_parity.txt": _parity("bbbb")}, "aaaa", dest)
    with pytest.raises(measure.Refused):   # a counter entry that names no hash at all
        measure.install({"r05_fp64_flops.json": json.dumps({"cfg2": {"source_hash": "aaaa"}, "cfg3": {"waves": 1.0}})}, "aaaa", dest)
    assert os.listdir(dest) == []
    measure.install({"r05_fuzz_parity.txt": _parity("aaaa"), "r05_full_scale_parity.txt": _parity("aaaa"), "r05_bench.json": "{}\n"}, "aaaa", dest)
    assert sorted(os.listdir(dest)) == ["r05_bench.json", "r05_full_scale_parity.txt", "r05_fuzz_parity.txt"]


def test_a_partial_counters_run_merges_only_into_a_file_of_the_same_library(tmp_path):
    path = tmp_path / "r05_pmc_traffic.json"
    before = json.dumps({"cfg1:draw": {"traffic_bytes": 1.0, "source_hash": "aaaa"}, "cfg2:draw": {"traffic_bytes": 2.0, "source_hash": "aaaa"}}, indent=1)
    path.write_text(before)
    new = {"cfg2:draw": {"traffic_bytes": 3.0, "source_hash": "bbbb"}}
    with pytest.raises(measure.Refused):   # cfg1's entry is of library aaaa
        measure.install({path.name: measure.merged(str(path), new)}, "bbbb", str(tmp_path))
    assert path.read_text() == before
    new["cfg2:draw"]["source_hash"] = "aaaa"
    measure.install({path.name: measure.merged(str(path), new)}, "aaaa", str(tmp_path))
    after = json.loads(path.read_text())
    assert list(after) == ["cfg1:draw", "cfg2:draw"] and after["cfg1:draw"]["traffic_bytes"] == 1.0 and after["cfg2:draw"] == new["cfg2:draw"]


# ------------------------------------------------------------------------------------------------------------ plan of a pass

MAIN_ONLY = "--warmup 3 --min-seconds 0 --sequence 8 --main-only"
# the bench.py command lines of the shell scripts this driver replaced (collect_pmc.sh, collect_fp64.sh, collect_sq.sh, collect_round.sh)
BENCH_COMMANDS = [f"python3 {REPO}/bench.py --workload {base}{rb} --mode {mode} --steps {steps} {MAIN_ONLY}"
                  for base, rb, steps in (("cfg1", "", 20), ("cfg2", "", 20), ("cfg2", " --road-boundary", 20), ("cfg3", "", 20),
                                          ("cfg3", " --road-boundary", 20), ("cfg3f", "", 20), ("cfg3f", " --road-boundary", 20),
                                          ("cfg4", "", 8), ("cfg4", " --road-boundary", 8), ("cfg5", "", 6))
                  for mode in ("draw", "draw", "fused")] + [
    "python3 bench.py --full --min-seconds 0.5",                       # (these two from the repository root)
    "python3 bench.py --full --min-seconds 0.5 --workload cfg2 --no-configs --no-cpu-baseline",
    f"python3 {REPO}/bench.py --full --min-seconds 0.5 --no-cpu-baseline",
    f"python3 {REPO}/bench.py --full --min-seconds 0.5 --no-cpu-baseline --no-configs",
    f"python3 {REPO}/bench.py --workload cfg3 --mode draw --steps 20 {MAIN_ONLY}",
    f"python3 {REPO}/bench.py --workload cfg3 --mode draw --steps 20 {MAIN_ONLY}",
    f"python3 {REPO}/bench.py --workload cfg5 --mode fused --steps 6 {MAIN_ONLY}",
    f"python3 {REPO}/bench.py --workload cfg5 --mode fused --steps 6 {MAIN_ONLY}"]
COUNTER_GROUPS = ["WRITE_SIZE", "FETCH_SIZE", "SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F64 SQ_WAVES"]


def test_plan_of_a_whole_pass(capsys, tmp_path):
    assert measure.main(["all", "--dry-run", "--out-root", str(tmp_path)]) == 0
    assert os.listdir(str(tmp_path)) == []
    lines = capsys.readouterr().out.splitlines()
    assert [l[3:] for l in lines if l.startswith("== ")] == ["counters", "bench", "trace", "sq", "parity"]
    stages, plan, kinds = {}, [], {}
    for l in lines:
        if l.startswith("== "):
            stage = stages.setdefault(l[3:], [])
        else:
            name, words = l.split(": ", 1)
            name, kind = name[:-1].split(" [")
            words = shlex.split(words)
            env = {w.split("=")[0]: w.split("=")[1] for w in words[:words.index("timeout")]}
            stage.append((name, env, words[words.index("timeout"):]))
            assert int(stage[-1][2][3]) == measure.LIMITS[kind] > 0, name   # the limit of the step's kind, from the table
            kinds[name] = kind
            plan.append(stage[-1])
    assert len(stages["counters"]) == 30 and len(stages["bench"]) == 3 and len(stages["sq"]) == 4 and len(stages["parity"]) == 7
    for name, env, argv in plan:
        assert argv[:3] == ["timeout", "-k", "10"] and int(argv[3]) > 0 and int(argv[3]) in measure.LIMITS.values(), name
        if argv[4] == "rocprofv3":
            assert env["TMPDIR"] == "/tmp" and argv[argv.index("--") + 1] == "python3", name
            if "--pmc" in argv:   # counters in a run of their own: no tracing beside them
                assert not [w for w in argv if w.endswith("-trace") or w == "--stats"], name
    assert [shlex.join(argv[argv.index("python3"):]) for _, _, argv in plan if {"bench.py", f"{REPO}/bench.py"} & set(argv)] == BENCH_COMMANDS
    pmc = [shlex.join(argv[argv.index("--pmc") + 1:argv.index("--output-format")]) for _, _, argv in stages["counters"]]
    assert pmc == COUNTER_GROUPS * 10
    assert {kinds[n] for n, _, _ in stages["counters"] + stages["sq"]} == {"pmc"} and {kinds[n] for n, _, _ in stages["parity"][:6]} == {"fuzz"}
    assert (kinds["bench"], kinds["bench_cfg2"], kinds["trace"], kinds["headline_trace"], kinds["full_scale"]) == \
        ("bench", "bench_cfg2", "trace", "trace", "full_scale")
    # the parity stage: the seed ranges and RP_AMD_* settings of the pass
    fuzz = [(env, argv[-2:]) for _, env, argv in stages["parity"][:6]]
    assert fuzz == [({}, ["100000", "30000"]),
                    ({"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_LAZY": "1", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}, ["130000", "10000"]),
                    ({"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_COST_KERNEL": "1", "RP_AMD_CHUNK_KERNEL": "0", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}, ["140000", "5000"]),
                    ({"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_CHUNK_KERNEL": "1", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}, ["145000", "10000"]),
                    ({"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_LAZY": "1", "RP_AMD_SWEEP": "1", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}, ["155000", "5000"]),
                    ({"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_G": "16", "RP_AMD_EVAL_BLOCK": "64", "RP_AMD_CHUNK_KERNEL": "0"}, ["160000", "3000"])]
    assert all(argv[4:6] == ["python3", "tests/sweeps/fuzz_parity.py"] for _, _, argv in stages["parity"][:6])
    assert stages["parity"][6][2][4:] == ["python3", "tests/sweeps/full_scale_parity.py"]


def test_soak_checks_every_sweep_before_it_starts_one(tmp_path, capsys):
    for bad in ("nonesuch:6:5", "default:6", "default:6:0", "default:6:30001"):
        assert measure.main(["soak", "default:1:5", bad, "--out-root", str(tmp_path)]) != 0
        assert "a fuzz run is" in capsys.readouterr().err
    assert os.listdir(str(tmp_path / "pass")) == []   # (no step, so no steps.jsonl and no log)
    # one title over consecutive runs of a launch path on adjoining seeds, as the soak's record has it
    assert measure.main(["soak", "default:1:5", "default:6:5", "default:20:5", "chunk:25:5", "--dry-run", "--out-root", str(tmp_path)]) == 0
    assert [l for l in capsys.readouterr().out.splitlines() if l.endswith(":")] == [
        "default launch paths, seeds 1 .. 10:", "default launch paths, seeds 20 .. 24:", "rp_chunk_kernel forced, seeds 25 .. 29:"]
