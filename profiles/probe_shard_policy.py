"""Option "shard_policy": what it costs a shard and what it buys.

  python profiles/probe_shard_policy.py [times] [cuts]

times: step time (wall clock around rp_plan, winner rows wanted, median of blocks that alternate the two policies) of the ranges
       [0, C/2), [0, C/4), [0, C/8) of cfg3 under "shard_policy" = 1 (producer of the cost bits by grid, the default) and = 0 (by range),
       with the producer each plan read back (options "last_lanes", "last_single_launch").
cuts:  the partitions of tests/test_shard_exchange.py under "shard_policy" = 0: per scene and partition the candidates whose cost bits
       differ from the unsharded plan's, and whether the combined winner or a counter moved (under = 1 the test asserts zero)."""
import os
import statistics
import sys
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "commonroad-reactive-planner_amd"), os.path.join(REPO, "tests")]
from commonroad_rp_amd import _capi  # noqa: E402
from commonroad_rp_amd import workloads as W  # noqa: E402


def times(blocks=5, steps=200, warmup=30):
    w = W.cfg3()
    ctx = _capi.RpContext(0)
    w.setup(ctx)
    C = w.inputs.n_candidates
    print(f"library {ctx._lib.rp_source_hash().decode()}, cfg3: {C} candidates, N = {w.inputs.params.N}; us per step, median of {blocks} blocks of {steps} plans"
          f" (min .. max of the block medians)")
    for div in (1, 2, 4, 8):
        hi = C // div
        med = {0: [], 1: []}
        prod = {}
        for b in range(blocks):
            for pol in ((1, 0) if b % 2 == 0 else (0, 1)):
                ctx.set_option("shard_policy", pol)
                for _ in range(warmup):
                    ctx.plan(w.inputs, 0, hi)
                t = []
                for _ in range(steps):
                    t0 = time.perf_counter()
                    out = ctx.plan(w.inputs, 0, hi)
                    t.append(time.perf_counter() - t0)
                med[pol].append(1e6 * statistics.median(t))
                prod[pol] = (ctx.get_option("last_lanes"), ctx.get_option("last_single_launch"), ctx.last_kernel(), ctx.last_path(), out.best_index)
        line = f"[0, C/{div}) = {hi:6d} candidates:"
        for pol in (1, 0):
            m = med[pol]
            line += f"  policy {pol}: {statistics.median(m):7.1f} ({min(m):.1f} .. {max(m):.1f}) lanes {prod[pol][0]} single launch {prod[pol][1]} {prod[pol][2]} path {prod[pol][3]}"
        line += f"  ratio 1/0 {statistics.median(med[1]) / statistics.median(med[0]):.3f}  winner {prod[1][4]} / {prod[0][4]}"
        print(line, flush=True)
    ctx.close()


def cuts():
    import test_shard_exchange as TX
    _capi.set_default_options({"shard_policy": 0})
    ctx = _capi.RpContext(0)
    print('partitions of tests/test_shard_exchange.py under "shard_policy" = 0 (candidates whose cost bits differ from the whole plan\'s)')
    for name in TX.CUT_SCENES:
        whole = TX._plan_whole(ctx, name)
        for tag, ranges in TX._cut_partitions(name):
            f = TX.compare_with_whole(ctx, name, whole, tag, ranges)
            moved = []
            if f.winner[0] != f.winner[1]:
                moved.append(f"winner {f.winner[1]} -> {f.winner[0]}")
            elif not f.winner_cost_bits_equal:
                moved.append("best_cost bits")
            if f.before[0] != f.before[1]:
                moved.append(f"collisions-before {f.before[1]} -> {f.before[0]}")
            if f.feasible[0] != f.feasible[1]:
                moved.append(f"feasible {f.feasible[1]} -> {f.feasible[0]}")
            print(f"{name:18s} {tag:18s} whole {whole.producer} shards {f.producers}: {f.cost_bits_differ:6d} of {len(whole.cost)} differ, status words "
                  f"{f.status_differ}; {', '.join(moved) if moved else 'result unmoved'}", flush=True)
    ctx.close()
    _capi.set_default_options(None)


if __name__ == "__main__":
    what = sys.argv[1:] or ["times", "cuts"]
    if "times" in what:
        times()
    if "cuts" in what:
        cuts()
