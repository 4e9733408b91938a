"""Partitions of the scenes of tests/_ladder.py into the candidate ranges of a sharded plan (used by tests/test_shard_combine_host.py,
which holds the host twin of the winner exchange to the unsharded selection on the oracle and asserts what this table covers, and
tests/test_shard_exchange.py, which does the same for rp_combine_kernel on the costs the device returned and holds every shard's
costs to the unsharded plan's).

A partition is a list of ranges [(lo, hi), ...] in rank order that covers [0, C) -- commonroad_rp_amd.distributed.shard_range for a
world size, or explicit cuts placed where a tie group, a single candidate or nothing at all ends up alone in a rank."""
import functools

import numpy as np

import _ladder as LD
from commonroad_rp_amd.distributed import shard_range

SMALL_SCENES = tuple(n for n in sorted(LD.SCENES) if LD.SCENES[n].n_candidates <= 10000)
HOST_WORLDS = (1, 2, 3, 5, 8, 64)
DEVICE_WORLDS = HOST_WORLDS + (33,)          # (64 is RP_COMBINE_MAX_WORLD; from 33 on thread 32 of rp_combine_kernel, which decides the owner, loads a message too)
CUT_WORLDS = (2, 3, 5, 16)                   # independence of the cut (module C)
EXPLICIT = ("at_5300", "first_alone", "behind_first_copy", "before_winner", "empty_middle", "empty_last")


def by_world(C, world):
    return [shard_range(C, r, world) for r in range(world)]


@functools.lru_cache(maxsize=None)
def explicit_cuts(name):
    """name of the cut -> ranges; per the ORACLE's costs where a cut depends on them"""
    sc, run = LD.oracle_run(name)
    C = sc.n_candidates
    groups = LD.tie_groups(run.cost, run.status & 3)
    k = int(groups[0][0]) + 1 if groups else 1        # directly behind the first copy of the cheapest tie group
    a = min(5300, C)
    w = max(1, min(C - 1, int(run.out.best_index)))   # directly before the winner: the copies of lower index (colliding ones) in the rank before
    return {
        "at_5300": [(0, a), (a, C)],
        "first_alone": [(0, 1), (1, C)],
        "behind_first_copy": [(0, k), (k, C)],
        "before_winner": [(0, w), (w, C)],
        "empty_middle": [(0, C // 3), (C // 3, C // 3), (C // 3, C)],
        "empty_last": [(0, C // 2), (C // 2, C), (C, C)],
    }


def partitions(name, worlds):
    """[(tag, ranges)]: shard_range at every world of ``worlds``, then the explicit cuts"""
    C = LD.oracle_run(name)[0].n_candidates
    return [(f"world{w}", by_world(C, w)) for w in worlds] + [(tag, explicit_cuts(name)[tag]) for tag in EXPLICIT]


def replicated(name):
    """[(tag, ranges)] that are NOT partitions: the whole grid planned by two ranks (redundant ranks; the same message gathered twice).
    The two messages are equal in (cost, index), the one case in which the order of the ranks decides the owner: the first one."""
    C = LD.oracle_run(name)[0].n_candidates
    return [("twice", [(0, C), (0, C)]), ("twice_around_empty", [(0, C), (C, C), (0, C)])]


def check_partition(ranges, C):
    assert ranges[0][0] == 0 and ranges[-1][1] == C and all(lo <= hi for lo, hi in ranges)
    assert all(ranges[r][1] == ranges[r + 1][0] for r in range(len(ranges) - 1))


def rank_of(ranges, index):
    """the rank whose range holds the candidate (-1: none / no candidate)"""
    return next((r for r, (lo, hi) in enumerate(ranges) if lo <= index < hi), -1)


def facts(cost, labels, ranges):
    """what a partition puts in front of the combine step, per these costs and labels (1 free, 3 colliding): a set of words"""
    wi, _, _ = LD.reference_selection(cost, labels)
    out = set()
    edges = np.array([lo for lo, _ in ranges[1:]] if len(ranges) > 1 else [], dtype=np.int64)
    for g in LD.tie_groups(cost, labels):
        if len(edges) and np.any((edges > g[0]) & (edges <= g[-1])):
            out.add("tie_group_across_a_cut")
            if wi >= 0 and cost[g[0]] == cost[wi]:
                out.add("winners_group_across_a_cut")
    for r, (lo, hi) in enumerate(ranges):
        if lo == hi:
            out.add("empty_last" if r == len(ranges) - 1 else ("empty_middle" if r > 0 else "empty_first"))
            continue
        lab = labels[lo:hi]
        if not np.any(lab == 1):
            out.add("rank_without_free")
        if not np.any((lab == 1) | (lab == 3)):
            out.add("rank_without_feasible")
    if wi < 0:
        out.add("no_winner")
    elif rank_of(ranges, wi) == len(ranges) - 1 and len(ranges) > 1:
        out.add("winner_in_last_rank")
    elif len(ranges) > 1 and rank_of(ranges, wi) > 0:
        out.add("winner_in_a_middle_rank")
    return out


WANTED = ("tie_group_across_a_cut", "winners_group_across_a_cut", "rank_without_free", "rank_without_feasible", "empty_middle", "empty_last",
          "no_winner", "winner_in_last_rank")
