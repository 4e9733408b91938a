"""The measurement pass of a round, and the counter probes, on one fail-stop step runner (standard library only).

    python3 profiles/measure.py <stage> --out-root DIR [--name NAME] [--dry-run]    (GPU box; outputs under <DIR>/<NAME>/, NAME "pass"
                                                                                     by default; DIR: a directory git ignores)

Stages, in the order of a pass (``all`` runs them in this order); each installs its records under profiles/ only after its last
step has succeeded, so a failed or interrupted stage leaves profiles/ as it found it:
    counters [workload ...]   rocprofv3 --pmc: WRITE_SIZE, FETCH_SIZE, FP64 classes    -> r05_pmc_traffic.json, r05_fp64_flops.json
    bench                     the full bench line, cfg2 as headline, plan() latency    -> r05_bench*.json, r05_plan_latency_ab.txt
    trace                     rocprofv3 --kernel-trace --stats of the bench line       -> r05_kernel_*, r05_headline_*, ...
    sq                        instruction-issue counters of cfg3 (draw), cfg5 (fused)  -> r05_sq_cfg3.json, r05_sq_cfg5_fused.json
    parity                    six fuzz sweeps and the full-scale sweep (tests/sweeps/) -> r05_fuzz_parity.txt, r05_full_scale_parity.txt
(counters come first: the bench line then carries `traffic` and the FP64 fraction of the library it ran on -- bench.py reports the
numbers of profiles/r05_*.json only when their source hash is the library's.)
Probes (they print their result and install nothing):
    lanes [workload] [steps] [mode]                                   lane utilisation of the evaluation kernel's vector instructions
    kernel-sq <workload> <nocoll|eager|prod> <eval16|lane|chunk|auto> <name>    SQ counters + durations of run_plans.py's kernels
    timeline <name> <workload[:mode]> ...                             step timelines (step_timeline.py) of workloads
    soak [path:first:n ...]                                           a longer fuzz comparison on seeds the pass does not use

Every step is a fresh child under `timeout -k 10 <limit>`, one at a time, recorded in <DIR>/<NAME>/steps.jsonl; after a step
that fails (non-zero status, or a GPU fault in its log) nothing else is started and the driver exits non-zero."""
import argparse
import collections
import csv
import functools
import glob
import json
import os
import shlex
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles")
ROUND = "r05"   # prefix of the judged records (bench.py and tests/test_bench_line.py name them)
FAULT_TEXT = "an illegal memory access was encountered"

# Seconds a step may take, by kind: about three times the wall time the step took on an MI355X (steps.jsonl; the longest of its kind,
# in seconds, beside each), rounded up to 30 s -- the boxes are shared and rocprofv3's start-up varies between runs.
LIMITS = {
    "pmc": 30,             # rocprofv3 --pmc of one bench.py --main-only run: 2.3 .. 3.6
    "pmc_plans": 30,       # rocprofv3 --pmc of run_plans.py: 2.5 .. 2.8
    "bench": 120,          # bench.py --full: 34.6
    "bench_cfg2": 30,      # bench.py --full --workload cfg2 --no-configs --no-cpu-baseline: 4.7
    "plan_latency": 30,    # probe_plan_latency_r05.py cfg2 cfg1: 2.3
    "trace": 60,           # rocprofv3 --kernel-trace --stats of bench.py --full: 15.2 (5.3 with --no-configs)
    "trace_plans": 30,     # rocprofv3 --kernel-trace --stats of run_plans.py: 2.5
    "trace_main": 30,      # rocprofv3 --kernel-trace of one bench.py --main-only run: 2.5
    "summary": 30,         # summarize_trace.py / step_timeline.py on a trace CSV (no GPU): 0.2 .. 1.5
    "fuzz": 600,           # fuzz_parity.py, up to 30 000 cases: 191.0 for 30 000 (6.4 .. 7.2 per 1 000)
    "full_scale": 60,      # full_scale_parity.py: 10.2
}
FUZZ_MAX_CASES = 30000

WORKLOADS = ("cfg1", "cfg2", "cfg2rb", "cfg3", "cfg3rb", "cfg3f", "cfg3frb", "cfg4", "cfg4rb", "cfg5")
STEPS = collections.defaultdict(lambda: 20, cfg4=8, cfg4rb=8, cfg5=6)
FP64_COUNTERS = "SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F64 SQ_WAVES".split()
SQ_GROUPS = {
    "a": "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_INSTS_SMEM".split(),
    "b": "SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_WAIT_INST_ANY SQ_INST_CYCLES_SALU SQ_ACTIVE_INST_ANY".split(),
    "c": "SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS SQ_WAIT_ANY SQ_INSTS_FLAT SQ_INSTS_VALU_MFMA_F64 SQ_WAIT_INST_LDS".split(),
}
#   SQ_INSTS_VALU           vector ALU instructions issued (wave level)
#   SQ_ACTIVE_INST_VALU     cycles waves spent executing VALU instructions (wave level, 4-cycle quads)
#   SQ_THREAD_CYCLES_VALU   the same counted per ACTIVE LANE: = SQ_ACTIVE_INST_VALU x 64 when every lane is on
LANE_COUNTERS = "SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU".split()
# launch paths of the fuzz sweeps: title, RP_AMD_* settings (the DEFAULTS rp_create gives a context's options: set for the whole child)
LAUNCH_PATHS = {
    "default": ("default launch paths", {}),
    "cost-ordered": ("cost-ordered stage forced", {"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_LAZY": "1", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}),
    "cost": ("rp_cost_kernel forced", {"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_COST_KERNEL": "1", "RP_AMD_CHUNK_KERNEL": "0",
                                       "RP_AMD_NO_AUTO_MATERIALIZE": "1"}),
    "chunk": ("rp_chunk_kernel forced", {"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_CHUNK_KERNEL": "1", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}),
    "sweep": ("bounded sweep forced", {"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_LAZY": "1", "RP_AMD_SWEEP": "1", "RP_AMD_NO_AUTO_MATERIALIZE": "1"}),
    "eval16": ("two-kernel path, 16 lanes, one wavefront per workgroup",
               {"RP_AMD_NO_FUSED_LON": "1", "RP_AMD_G": "16", "RP_AMD_EVAL_BLOCK": "64", "RP_AMD_CHUNK_KERNEL": "0"}),
}
PARITY_SWEEPS = (("default", 100000, 30000), ("cost-ordered", 130000, 10000), ("cost", 140000, 5000), ("chunk", 145000, 10000),
                 ("sweep", 155000, 5000), ("eval16", 160000, 3000))
SOAK_SWEEPS = ("default:300000:25000", "default:325000:25000", "default:350000:25000", "default:375000:25000",
               "cost-ordered:400000:30000", "chunk:430000:30000", "sweep:460000:20000", "cost:480000:20000")


# ---------------------------------------------------------------------------------------------------------------- the step runner

class StepFailed(Exception):
    pass


class Refused(Exception):
    pass


class Runner:
    """Starts the children of a pass, one after the other, each under its time limit; the only place that starts a process."""

    def __init__(self, out, dry_run=False):
        self.out, self.dry_run = out, dry_run
        if not dry_run:
            os.makedirs(out, exist_ok=True)

    def step(self, name, kind, argv, env=None, cwd=ROOT, merge_err=False):
        """Run ``argv`` (from the repository root unless ``cwd`` says otherwise) with stdout in <out>/<name>.out and stderr in
        <out>/<name>.err -- with ``merge_err`` in the former too, as `2>&1`; returns the former's path."""
        limit = LIMITS[kind]
        argv = ["timeout", "-k", "10", str(limit)] + [str(a) for a in argv]
        log, err = os.path.join(self.out, name + ".out"), os.path.join(self.out, name + ".err")
        if self.dry_run:
            print(f"{name} [{kind}]: " + " ".join([f"{k}={v}" for k, v in (env or {}).items()] + [shlex.join(argv)]))
            return log
        t0 = time.time()
        with open(log, "w") as o, open(err, "w") as e:
            status = subprocess.run(argv, stdout=o, stderr=subprocess.STDOUT if merge_err else e, stdin=subprocess.DEVNULL, cwd=cwd, env=dict(os.environ, **(env or {}))).returncode
        with open(os.path.join(self.out, "steps.jsonl"), "a") as f:
            f.write(json.dumps({"step": name, "argv": argv, "limit": limit, "status": status, "seconds": round(time.time() - t0, 1)}) + "\n")
        faulted = [p for p in (log, err) if FAULT_TEXT in open(p, errors="replace").read()]
        if status != 0 or faulted:
            raise StepFailed(f"step {name} failed: status {status}{', GPU fault reported' if faulted else ''}; log {(faulted or [log if merge_err else err])[0]}")
        return log

    def rocprof(self, name, kind, options, out_dir, program):
        """rocprofv3 <options> --output-format csv -d <out_dir> -- <program> (from /tmp: the profiler leaves scratch files)"""
        return self.step(name, kind, ["rocprofv3"] + options + ["--output-format", "csv", "-d", out_dir, "--"] + program,
                         env={"TMPDIR": "/tmp"}, cwd="/tmp")


def main_only(workload, steps, mode, warmup=3, min_seconds=0, sequence=8):
    """bench.py's timed region of one workload alone; <workload>rb: the workload with its road boundary"""
    rb = ["--road-boundary"] if workload.endswith("rb") else []
    return ["python3", os.path.join(ROOT, "bench.py"), "--workload", workload[:-2] if rb else workload] + rb + \
        ["--mode", mode, "--steps", steps, "--warmup", warmup, "--min-seconds", min_seconds, "--sequence", sequence, "--main-only"]


def without_noise(path):
    return [l for l in open(path).read().splitlines() if "amdgpu.ids" not in l]


def first_file(pattern):
    """the first match, as `ls | head -1` (the pattern itself where there is none: a dry run, or a step that will then fail)"""
    return (sorted(glob.glob(pattern)) or [pattern])[0]


# ------------------------------------------------------------------------------------------------------------ counter summaries

# the kernels that evaluate a batch (one of them per plan: rp_last_kernel) and the ones around it
MAIN_KERNELS = ("rp_eval_kernel", "rp_cost_kernel", "rp_chunk_kernel")
SIDE_KERNELS = ("rp_lon_kernel", "rp_select_kernel", "rp_finalize_kernel")


def rows_of(directory):
    """the rows of rocprofv3's counter_collection CSVs of one pass"""
    out = []
    for f in glob.glob(os.path.join(directory, "*", "*_counter_collection.csv")):
        out += list(csv.DictReader(open(f)))
    return out


def short(kernel_name):
    """template instance without the argument list: 'void rp_eval_kernel<16, true, ...>'"""
    return kernel_name.split("(")[0]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def by_kernel(rows, names=MAIN_KERNELS, largest_grid=True):
    """{kernel instance: {counter: [values]}} over the launches of ``names``; with ``largest_grid`` only the launches of the largest
    grid among them (the batch's evaluation launch -- the winner's re-evaluation and the cost-ordered rounds are smaller)."""
    rows = [r for r in rows if any(n in r["Kernel_Name"] for n in names)]
    vals = collections.defaultdict(lambda: collections.defaultdict(list))
    if not rows:
        return vals
    gmax = max(int(r["Grid_Size"]) for r in rows)
    for r in rows:
        if not largest_grid or int(r["Grid_Size"]) == gmax:
            vals[short(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return vals


def main_kernel_of(bench_json):
    """the kernel family the bench line says evaluated the batch (roofline.kernel <- rp_last_kernel); all of them if the line has none"""
    try:
        k = json.load(open(bench_json))["roofline"]["kernel"]
        return (k,) if k in MAIN_KERNELS else MAIN_KERNELS
    except Exception:
        return MAIN_KERNELS


def traffic_entry(out, workload, mode, bench_json):
    """Median WRITE_SIZE / FETCH_SIZE (KB) of the launches that evaluate the batch (largest grid) and of the kernels around them ->
    bytes per launch; from <out>/w and <out>/r (separate passes).  The variant is picked ONCE -- the instance with the largest median
    WRITE_SIZE (the bench's timed region runs the state-writing variant; the winner pass and the cost-ordered rounds are other
    instances or smaller grids) -- and both counters are read from that same named instance.  FETCH_SIZE is doubled (gfx950 reports
    half the bytes of wide coalesced reads); WRITE_SIZE is taken as is (exact for 16-B-per-lane streaming stores)."""
    family = main_kernel_of(bench_json)   # (the bench line of the WRITE_SIZE pass)
    passes = {"WRITE_SIZE": rows_of(os.path.join(out, "w")), "FETCH_SIZE": rows_of(os.path.join(out, "r"))}
    wv = by_kernel(passes["WRITE_SIZE"], family)
    if not wv:
        raise Refused(f"no WRITE_SIZE rows of {family} under {out}")
    name = max(wv, key=lambda k: median(wv[k]["WRITE_SIZE"]))
    rv = by_kernel(passes["FETCH_SIZE"], family)
    if name not in rv:
        raise Refused(f"{name} has no FETCH_SIZE launches of the largest grid: {sorted(rv)}")
    res = {"WRITE_SIZE": {"kernel": name, "median_KB": median(wv[name]["WRITE_SIZE"]), "n": len(wv[name]["WRITE_SIZE"])},
           "FETCH_SIZE": {"kernel": name, "median_KB": median(rv[name]["FETCH_SIZE"]), "n": len(rv[name]["FETCH_SIZE"])}}
    w = res["WRITE_SIZE"]["median_KB"] * 1024.0
    r = res["FETCH_SIZE"]["median_KB"] * 1024.0 * 2.0
    # the other kernels of a step: per instance, median bytes per launch (same corrections), every grid size
    side = {}
    for tag, factor in (("WRITE_SIZE", 1.0), ("FETCH_SIZE", 2.0)):
        for k, d in by_kernel(passes[tag], SIDE_KERNELS, largest_grid=False).items():
            side.setdefault(k, {})[tag.lower().replace("_size", "_bytes")] = median(d[tag]) * 1024.0 * factor
            side[k]["launches"] = len(d[tag])
    return {"workload": workload, "mode": mode, "kernel": name, "write_bytes": w, "fetch_bytes_corrected_x2": r, "traffic_bytes": w + r,
            "detail": res, "other_kernels": side}


def fp64_entry(out, workload, mode, bench_json):
    """FP64 instruction classes of the launches that evaluate the batch (largest grid; <out>/a) -> flops per (candidate, step):
    64 lanes x (ADD + MUL + TRANS + 2 x FMA) per wavefront instruction, all lanes counted (a lane that is masked off still occupies
    its slot of the FP64 pipe, which is what the "valu" roofline of bench.py prices)."""
    line = json.load(open(bench_json))
    cand, n1 = float(line["config"]["candidates_per_step"]), int(line["config"]["horizon_steps"]) + 1
    vals = by_kernel(rows_of(os.path.join(out, "a")), main_kernel_of(bench_json))
    if not vals:
        raise Refused(f"no counter rows of {main_kernel_of(bench_json)} under {out}")
    name, d = max(vals.items(), key=lambda kv: len(kv[1].get("SQ_WAVES", [])))
    med = {c: median(v) for c, v in d.items()}
    inst = {k: med.get(f"SQ_INSTS_VALU_{k}_F64", 0.0) for k in ("ADD", "MUL", "FMA", "TRANS")}
    flops = 64.0 * (inst["ADD"] + inst["MUL"] + inst["TRANS"] + 2.0 * inst["FMA"])
    return {"workload": workload, "mode": mode, "kernel": name, "candidates": cand, "steps": n1, "wave_instructions": inst,
            "waves": med.get("SQ_WAVES"), "flops_per_launch": flops, "flops_per_candidate_step": flops / (cand * n1),
            "model": "64 lanes x (ADD_F64 + MUL_F64 + TRANS_F64 + 2 FMA_F64) wavefront instructions counted by the SQ block (rocprofv3 --pmc), "
                     "median launch, / (candidates x (N + 1))"}


def sq_kernels(out, bench_json):
    """Median SQ counter values of the launches that evaluate the batch (largest grid; <out>/a and <out>/b) and per-wave
    instruction counts, per kernel instance."""
    vals = by_kernel(rows_of(os.path.join(out, "a")) + rows_of(os.path.join(out, "b")), main_kernel_of(bench_json))
    res = {}
    for k, d in vals.items():
        res[k] = {c: median(v) for c, v in d.items()}
        w = res[k].get("SQ_WAVES")
        if w:
            res[k]["per_wave"] = {c: round(v / w, 1) for c, v in res[k].items() if c.startswith("SQ_INSTS")}
    return res


def lane_kernels(out, bench_json):
    """lane utilisation (as rocprof's VALUUtilization) = SQ_THREAD_CYCLES_VALU / (SQ_ACTIVE_INST_VALU x 64), per kernel instance"""
    res = {}
    for k, d in by_kernel(rows_of(os.path.join(out, "a")), main_kernel_of(bench_json)).items():
        m = {c: median(v) for c, v in d.items()}
        if m.get("SQ_ACTIVE_INST_VALU"):
            m["lane_utilisation"] = round(m.get("SQ_THREAD_CYCLES_VALU", 0.0) / (64.0 * m["SQ_ACTIVE_INST_VALU"]), 4)
        if m.get("SQ_WAVES"):
            m["valu_insts_per_wave"] = round(m.get("SQ_INSTS_VALU", 0.0) / m["SQ_WAVES"], 1)
        res[k] = m
    return res


def kernel_sq_lines(out):
    """Per-kernel medians of the counters of <out>/a, b, c (every launch; the largest grid is named) + trace durations of <out>/t."""
    vals = collections.defaultdict(lambda: collections.defaultdict(list))
    grid = {}
    for f in glob.glob(os.path.join(out, "[abc]", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = short(r["Kernel_Name"])
            vals[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
            grid[k] = max(grid.get(k, 0), int(r["Grid_Size"]))
    dur = collections.defaultdict(list)
    for f in glob.glob(os.path.join(out, "t", "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            dur[short(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = []
    for k in sorted(vals):
        c = {n: median(v) for n, v in vals[k].items()}
        w = c.get("SQ_WAVES", 0) or 1
        d = median(dur[k]) if dur.get(k) else float("nan")
        lines.append(f"{k[:70]:70s} grid {grid[k]:8d} dur {d:8.1f} us | waves {w:8.0f} | per wave: VALU {c.get('SQ_INSTS_VALU',0)/w:8.1f} SALU {c.get('SQ_INSTS_SALU',0)/w:7.1f} "
                     f"LDS {c.get('SQ_INSTS_LDS',0)/w:6.1f} VMEM_RD {c.get('SQ_INSTS_VMEM_RD',0)/w:6.1f} VMEM_WR {c.get('SQ_INSTS_VMEM_WR',0)/w:6.1f} SMEM {c.get('SQ_INSTS_SMEM',0)/w:6.1f} FLAT {c.get('SQ_INSTS_FLAT',0)/w:6.1f} | "
                     f"wave_cycles/wave {c.get('SQ_WAVE_CYCLES',0)/w:9.0f} busy_cycles {c.get('SQ_BUSY_CYCLES',0):9.0f} active_valu/wave {c.get('SQ_ACTIVE_INST_VALU',0)/w:8.0f} "
                     f"wait_inst_any/wave {c.get('SQ_WAIT_INST_ANY',0)/w:9.0f} wait_any/wave {c.get('SQ_WAIT_ANY',0)/w:9.0f} inst_cycles_vmem/wave {c.get('SQ_INST_CYCLES_VMEM',0)/w:8.0f} active_vmem/wave {c.get('SQ_ACTIVE_INST_VMEM',0)/w:8.0f} "
                     f"active_lds/wave {c.get('SQ_ACTIVE_INST_LDS',0)/w:7.0f} wait_lds/wave {c.get('SQ_WAIT_INST_LDS',0)/w:7.0f}")
    return lines


# ------------------------------------------------------------------------------------------------------------------- installing

@functools.lru_cache(None)
def library_hash():
    """hash of the sources of the library the children load (rp_source_hash)"""
    sys.path[:0] = [os.path.join(ROOT, "commonroad-reactive-planner_amd")]
    from commonroad_rp_amd import _capi
    return _capi.source_hash()


def named_hashes(name, text):
    """the source hashes a record names: every entry of the two counter files, the SQ records' own, the parity records' first line"""
    if name.endswith(("_pmc_traffic.json", "_fp64_flops.json")):
        return {e.get("source_hash") if isinstance(e, dict) else None for e in json.loads(text).values()}
    if name.startswith(ROUND + "_sq_"):
        return {json.loads(text).get("source_hash")}
    if name.endswith("_parity.txt"):
        return {text.split("\n", 1)[0].rsplit("library source hash ", 1)[-1].strip()}
    return set()


def install(records, lib_hash, dest=PROFILES):
    """Write {file name: text} into ``dest``, all or nothing: refused unless every hash the records name is the loaded library's;
    each file is written beside its target, then all are moved into place."""
    named = {n: named_hashes(n, t) for n, t in records.items()}
    other = {n: sorted(map(str, h)) for n, h in named.items() if h - {lib_hash}}
    if other:
        raise Refused(f"not installing {sorted(records)}: the loaded library is {lib_hash}, but records name {other}")
    for n, t in records.items():   # (every file written before the first is moved)
        with open(os.path.join(dest, n + ".tmp"), "w") as f:
            f.write(t)
    for n in records:
        os.replace(os.path.join(dest, n + ".tmp"), os.path.join(dest, n))


def merged(path, entries):
    """the entries of the counter file ``path`` (if there is one) with ``entries`` put over them, as JSON text"""
    try:
        allr = json.load(open(path))
    except Exception:
        allr = {}
    allr.update(entries)
    return json.dumps(allr, indent=1)


def run_stage(stage, run, lib_hash=None, dest=PROFILES):
    """One stage or probe: its steps, then -- only if every one succeeded -- its records (a probe has none); returns the exit status."""
    name = getattr(stage, "func", stage).__name__
    try:
        if run.dry_run:
            print(f"== {name}")
        records = stage(run)
        if records and not run.dry_run:
            for n, t in records.items():
                with open(os.path.join(run.out, n), "w") as f:
                    f.write(t)
            install(records, lib_hash or library_hash(), dest)
            print(f"{name}: installed {' '.join(sorted(records))}", flush=True)
        return 0
    except (StepFailed, Refused) as e:
        print(f"{name}: {e}\nnothing installed, nothing further started", file=sys.stderr)
        return 1


# ----------------------------------------------------------------------------------------------------------------------- stages

def counters(run, workloads=WORKLOADS):
    traffic, fp64 = {}, {}
    lib = None if run.dry_run else library_hash()
    for wl in workloads:
        n, pmc, f64 = STEPS[wl], os.path.join(run.out, f"pmc_{wl}_draw"), os.path.join(run.out, f"fp64_{wl}_fused")
        # (separate passes for WRITE_SIZE and FETCH_SIZE; no trace domains combined with --pmc)
        bench_w = run.rocprof(f"pmc_{wl}_write", "pmc", ["--pmc", "WRITE_SIZE"], os.path.join(pmc, "w"), main_only(wl, n, "draw"))
        run.rocprof(f"pmc_{wl}_fetch", "pmc", ["--pmc", "FETCH_SIZE"], os.path.join(pmc, "r"), main_only(wl, n, "draw"))
        bench_f = run.rocprof(f"fp64_{wl}", "pmc", ["--pmc"] + FP64_COUNTERS, os.path.join(f64, "a"), main_only(wl, n, "fused"))
        if not run.dry_run:
            traffic[f"{wl}:draw"] = dict(traffic_entry(pmc, wl, "draw", bench_w), source_hash=lib)   # key read back by bench.py
            fp64[wl] = dict(fp64_entry(f64, wl, "fused", bench_f), source_hash=lib)
            print(f"{wl} counters done", flush=True)
    return {f"{ROUND}_pmc_traffic.json": merged(os.path.join(PROFILES, f"{ROUND}_pmc_traffic.json"), traffic),
            f"{ROUND}_fp64_flops.json": merged(os.path.join(PROFILES, f"{ROUND}_fp64_flops.json"), fp64)}


def bench(run):
    # (--min-seconds 0.5: the headline repeats its K-step regions for 0.5 s, as the records of earlier rounds did)
    rec = {}
    bench_py = ["python3", "bench.py", "--full", "--min-seconds", "0.5"]
    # cfg2 as the headline workload (the headline of rounds 1-2; carries plan() latency on cfg2)
    for tag, kind, extra in (("bench", "bench", []), ("bench_cfg2", "bench_cfg2", ["--workload", "cfg2", "--no-configs", "--no-cpu-baseline"])):
        line = run.step(tag, kind, bench_py + extra)
        if not run.dry_run:
            rec[f"{ROUND}_{tag}.json"] = open(line).read()
            detail = json.loads(rec[f"{ROUND}_{tag}.json"]).get("detail")   # where bench.py put the full record, from the root
            if not detail:
                raise Refused(f"the bench line of {tag} names no detail record: {line}")
            rec[f"{ROUND}_{tag}_detail.json"] = open(os.path.join(ROOT, detail)).read()
    # plan() in closed loop with the cycle's call made by the binding's extension module / through ctypes, on this box
    lat = run.step("plan_latency", "plan_latency", ["python3", "profiles/probe_plan_latency_r05.py", "cfg2", "cfg1"], merge_err=True)
    if not run.dry_run:
        rec[f"{ROUND}_plan_latency_ab.txt"] = "\n".join(without_noise(lat)) + "\n"
    return rec


def trace(run):
    rec = {}
    bench_py = ["python3", os.path.join(ROOT, "bench.py"), "--full", "--min-seconds", "0.5", "--no-cpu-baseline"]
    summary = lambda name, script, csv_file, *a, **kw: run.step(name, "summary", ["python3", os.path.join(PROFILES, script), csv_file] + list(a), **kw)
    # the headline alone (no side configurations: cfg3rb / cfg3frb launch the same kernel instance on the same grid as the headline, so
    # the averages of the full line's trace mix three workloads): the kernel durations bench.py's headline `kernel_ms` has to agree with
    for tag, extra in (("", []), ("headline_", ["--no-configs"])):
        prof = os.path.join(run.out, f"prof_{tag}trace")
        line = run.rocprof(f"{tag}trace", "trace", ["--kernel-trace", "--stats"], prof, bench_py + extra)
        trace_csv = first_file(os.path.join(prof, "*", "*kernel_trace.csv"))
        outs = {f"{ROUND}_{tag}bench_under_rocprof.json": line,
                f"{ROUND}_{tag}kernel_trace_summary.txt": summary(f"{tag}trace_summary", "summarize_trace.py", trace_csv)}
        if tag:
            outs[f"{ROUND}_headline_step_timeline.txt"] = summary("headline_step_timeline", "step_timeline.py", trace_csv, merge_err=True)
            outs[f"{ROUND}_production_step_timeline.txt"] = summary("production_step_timeline", "step_timeline.py", trace_csv, "production", merge_err=True)
        else:
            outs[f"{ROUND}_kernel_stats.csv"] = first_file(os.path.join(prof, "*", "*kernel_stats.csv"))
        if not run.dry_run:
            rec.update({n: open(p).read() for n, p in outs.items()})
            shutil.rmtree(prof)   # (the traces of a full bench line are hundreds of MB)
    return rec


def sq(run):
    rec = {}
    lib = None if run.dry_run else library_hash()
    for wl, mode, record in (("cfg3", "draw", f"{ROUND}_sq_cfg3.json"), ("cfg5", "fused", f"{ROUND}_sq_cfg5_fused.json")):
        out = os.path.join(run.out, f"sq_{wl}_{mode}")
        lines = [run.rocprof(f"sq_{wl}_{g}", "pmc", ["--pmc"] + SQ_GROUPS[g], os.path.join(out, g), main_only(wl, STEPS[wl], mode)) for g in "ab"]
        if not run.dry_run:
            rec[record] = json.dumps({"workload": wl, "source_hash": lib, "kernels": sq_kernels(out, lines[0])}, indent=1) + "\n"
    return rec


def fuzz_sweeps(run, sweeps, with_settings):
    """fuzz_parity.py once per (launch path, first seed, cases), every one checked before the first is started: a title line per
    launch path and seed range (one over consecutive runs of a path on adjoining seeds), then each run's last line, as they come"""
    for path, first, n in sweeps:
        if path not in LAUNCH_PATHS or not 0 < n <= FUZZ_MAX_CASES:
            raise Refused(f"a fuzz run is <{'|'.join(LAUNCH_PATHS)}>:<first seed>:<1 .. {FUZZ_MAX_CASES} cases> (the step's time limit "
                          f"is sized for that many), not {path}:{first}:{n}")

    def lines():
        for i, (path, first, n) in enumerate(sweeps):
            title, env = LAUNCH_PATHS[path]
            if i == 0 or sweeps[i - 1][0] != path or sum(sweeps[i - 1][1:]) != first:
                end = first + n
                for p, f, m in sweeps[i + 1:]:
                    if p != path or f != end:
                        break
                    end += m
                settings = f" ({' '.join(f'{k}={v}' for k, v in env.items())})" if with_settings and env else ""
                yield f"{title}{settings}, seeds {first} .. {end - 1}:"
            log = run.step(f"fuzz_{path}_{first}", "fuzz", ["python3", "tests/sweeps/fuzz_parity.py", first, n], env=env, merge_err=True)
            yield from [] if run.dry_run else without_noise(log)[-1:]
    return lines()


def parity(run):
    """the sweeps outside pytest on the default launch paths and with the other paths forced; every record names the library"""
    lib = None if run.dry_run else library_hash()
    fuzz = [f"Fuzz sweeps (tests/sweeps/fuzz_parity.py) on MI355X, library source hash {lib}"] + list(fuzz_sweeps(run, PARITY_SWEEPS, True))
    full = run.step("full_scale", "full_scale", ["python3", "tests/sweeps/full_scale_parity.py"], merge_err=True)
    if run.dry_run:
        return {}
    full = [f"Full benchmark workloads against the oracle's brute force (tests/sweeps/full_scale_parity.py) on MI355X, library source hash {lib}"] \
        + without_noise(full)
    print("\n".join(fuzz[-3:] + full[-3:]))
    return {f"{ROUND}_fuzz_parity.txt": "\n".join(fuzz) + "\n", f"{ROUND}_full_scale_parity.txt": "\n".join(full) + "\n"}


STAGES = {"counters": counters, "bench": bench, "trace": trace, "sq": sq, "parity": parity}


# ----------------------------------------------------------------------------------------------------------------------- probes

def lanes(run, workload, steps, mode):
    out = os.path.join(run.out, f"lanes_{workload}_{mode}")
    line = run.rocprof(f"lanes_{workload}_{mode}", "pmc", ["--pmc"] + LANE_COUNTERS, os.path.join(out, "a"), main_only(workload, steps, mode))
    if not run.dry_run:
        print(json.dumps({"workload": workload, "mode": mode, "source_hash": library_hash(), "kernels": lane_kernels(out, line)}, indent=1))


def kernel_sq(run, workload, mode, kernel):
    """SQ counters of run_plans.py's kernels for one (workload, mode, kernel) -- separate passes, counters only -- and a kernel trace"""
    out = os.path.join(run.out, f"{workload}_{mode}_{kernel}")
    plans = lambda n: ["python3", os.path.join(PROFILES, "run_plans.py"), workload, mode, kernel, n]
    for g in "abc":
        run.rocprof(f"{workload}_{mode}_{kernel}_{g}", "pmc_plans", ["--pmc"] + SQ_GROUPS[g], os.path.join(out, g), plans(6))
    run.rocprof(f"{workload}_{mode}_{kernel}_t", "trace_plans", ["--kernel-trace", "--stats"], os.path.join(out, "t"), plans(20))
    if not run.dry_run:
        text = "\n".join(kernel_sq_lines(out)) + "\n"
        open(os.path.join(out, "summary.txt"), "w").write(text)
        print(text, end="")


def timeline(run, specs):
    """step timelines of workloads from rocprofv3 kernel traces of the headline region"""
    timelines = os.path.join(run.out, "step_timelines.txt")
    for spec in specs:
        wl, mode = (spec.split(":") + ["draw"])[:2]
        prof = os.path.join(run.out, f"trace_{wl}")
        run.rocprof(f"trace_{wl}", "trace_main", ["--kernel-trace"], prof, main_only(wl, 50, mode, warmup=10, min_seconds=0.1, sequence=16))
        steps = run.step(f"step_timeline_{wl}", "summary",
                         ["python3", os.path.join(PROFILES, "step_timeline.py"), first_file(os.path.join(prof, "*", "*kernel_trace.csv"))])
        if not run.dry_run:
            with open(timelines, "a") as f:
                f.write(f"== {wl} {mode}\n" + open(steps).read())
            shutil.rmtree(prof)
    if not run.dry_run:
        print(open(timelines).read(), end="")


def soak(run, sweeps):
    """fuzz_parity.py (random small plans, HIP path against the oracle) on seeds the pass does not use"""
    try:
        sweeps = [(p, int(first), int(n)) for p, first, n in (s.split(":") for s in sweeps)]
    except ValueError:
        raise Refused(f"a fuzz run is <path>:<first seed>:<cases>: {' '.join(sweeps)}")
    lines = fuzz_sweeps(run, sweeps, False)
    if not run.dry_run:
        print(f"Fuzz soak on MI355X, library source hash {library_hash()}", flush=True)
    for line in lines:   # (as soon as there is one: a run of 25 000 cases takes about three minutes)
        print(line, flush=True)


def main(argv=None):
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--dry-run", action="store_true", help="print the steps, start nothing")
    common.add_argument("--out-root", required=True, metavar="DIR", help="outputs (logs, raw CSVs, steps.jsonl) go to <DIR>/<name>/")
    named = argparse.ArgumentParser(add_help=False, parents=[common])
    named.add_argument("--name", default="pass")
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    for s in list(STAGES) + ["all"]:
        p = sub.add_parser(s, parents=[named])
        if s == "counters":
            p.add_argument("workloads", nargs="*", default=list(WORKLOADS), help=f"of {' '.join(WORKLOADS)} (default: all; fewer are "
                           "merged into the installed files)")
    p = sub.add_parser("lanes", parents=[named])
    p.add_argument("workload", nargs="?", default="cfg3")
    p.add_argument("steps", nargs="?", default="20")
    p.add_argument("mode", nargs="?", default="fused")
    p = sub.add_parser("kernel-sq", parents=[common])
    p.add_argument("workload")
    p.add_argument("mode", choices=["nocoll", "eager", "prod"])
    p.add_argument("kernel", choices=["eval16", "lane", "chunk", "auto"])
    p.add_argument("name")
    p = sub.add_parser("timeline", parents=[common])
    p.add_argument("name")
    p.add_argument("specs", nargs="+", metavar="workload[:mode]")
    p = sub.add_parser("soak", parents=[named])
    p.add_argument("sweeps", nargs="*", metavar="path:first:n", default=list(SOAK_SWEEPS), help=f"path: one of {' '.join(LAUNCH_PATHS)}")
    a = ap.parse_args(argv)
    run = Runner(os.path.abspath(os.path.join(a.out_root, a.name)), a.dry_run)   # (absolute: rocprofv3 runs from /tmp)
    if a.command == "all":
        for stage in STAGES.values():
            if run_stage(stage, run):
                return 1
        return 0
    if a.command == "counters":
        if set(a.workloads) - set(WORKLOADS):
            ap.error(f"counters: workloads are {' '.join(WORKLOADS)}")
        return run_stage(functools.partial(counters, workloads=a.workloads), run)
    if a.command in STAGES:
        return run_stage(STAGES[a.command], run)
    if a.command == "lanes":
        return run_stage(functools.partial(lanes, workload=a.workload, steps=a.steps, mode=a.mode), run)
    if a.command == "kernel-sq":
        return run_stage(functools.partial(kernel_sq, workload=a.workload, mode=a.mode, kernel=a.kernel), run)
    if a.command == "timeline":
        return run_stage(functools.partial(timeline, specs=a.specs), run)
    return run_stage(functools.partial(soak, sweeps=a.sweeps), run)


if __name__ == "__main__":
    sys.exit(main())
