"""A scene family with exact cost ties and a dial for where the first free candidate sits in the cost order (used by
tests/test_ladder_scenes.py, which holds the table to its coverage on the oracle, and tests/test_selection_edges.py, which runs
it through the selection chain of the library: block partials -> rp_fold_partials_kernel -> rp_finalize_kernel / rp_select_kernel, the
cost-ordered stage and the bounded sweep).

Straight reference path along x, velocity keeping from (s, v) = (10, 10), N = 20 (21 steps: two step blocks, the smallest horizon
at which rp_chunk_kernel applies and the sweep is not the one-block instance).  The grids carry DUPLICATE samples
  T = [2.0, 1.6, 2.0, 1.6, ...]      (the 1.6-s candidates also run the horizon extension)
  L = tile(linspace(L_lo, L_hi, nLu), rL)
  D = tile(linspace(D_lo, D_hi, nDu), rD)
so that candidates that are the same arithmetic on the same inputs -- bit-equal in every kernel and in the oracle -- sit at
controlled index distances (D copies nDu apart, L copies nLu * nD apart, T copies 2 * nL * nD apart).  One static rectangle across
the road ahead of the ego, [x_near + 9, off, 0, 9, w]: the cheap candidates (small |d|) run into it, so its half width w, its
lateral offset and its distance dial how many feasible candidates sort before the first free one.  nDu is chosen so that
linspace(-3, 3.3, nDu) has no +/- pairs (candidates mirrored in d have equal costs by symmetry of the cost terms, which would merge
tie groups); the mirror scene wants exactly that and takes a symmetric grid and a one-sided wall.

reference_selection() is the plain-NumPy statement of the selection; stage_model() restates, on the host, which candidates the
lists of the cost-ordered stage hold (rp_kernels.h: lazy_bin, rp_lazy_hist_kernel) and what run_lazy (rp_host.hip) makes of them."""
import dataclasses
import functools

import numpy as np

from commonroad_rp_amd import workloads as W
from commonroad_rp_amd._capi import PlanInputs, make_cost, make_params
from commonroad_rp_amd.collision import ObstacleTables

DT, N_STEPS = 0.1, 20
LIST_CAP = (1024, 4096, 16384)       # rp_host.hip: kLazyCap
LIST_TARGET = (128, 1024, 8192)      # rp_host.hip: kLazyTarget (cumulative)
LIST_TOTAL = sum(LIST_CAP)           # 21 504
SELECT_ABOVE = 1 << 14               # rp_kernels.h: RP_FINALIZE_MAX -- larger batches take rp_select_kernel
SEL_SLICE = 2048                     # rp_kernels.h: RP_SEL_SLICE
FOLD_SLOTS = 256                     # rp_host.hip: kFoldPartials
SWEEP_MIN_PER_CU = 512               # rp_host.hip: kSweepMinPerCU


@dataclasses.dataclass(frozen=True)
class SceneSpec:
    nT: int
    nLu: int
    rL: int
    nDu: int
    rD: int
    w: float                 # half width of the wall
    off: float = 0.0         # its lateral offset
    x_near: float = 30.0     # its near face
    L_lo: float = 8.0
    L_hi: float = 12.0
    D_lo: float = -3.0
    D_hi: float = 3.3
    a_max: float = None      # None: the vehicle's
    n_steps: int = 20        # N of the plan (N + 1 steps)

    @property
    def n_candidates(self):
        return self.nT * self.nLu * self.rL * self.nDu * self.rD


_G8 = dict(nT=6, nLu=11, rL=3, nDu=21, rD=2)        # 8 316 candidates (21, not the 22 lateral samples of a 0.3-m grid: those come in +/- pairs)
_G48 = dict(nT=8, nLu=33, rL=2, nDu=45, rD=2)       # 47 520: beyond the one-workgroup epilogue, below the sweep's size
_G135 = dict(nT=12, nLu=50, rL=2, nDu=57, rD=2)     # 136 800: from 512 candidates per CU on exhausted lists hand over to the sweep
_GOV = dict(nT=12, nLu=1, rL=60, nDu=3, rD=3, L_lo=10.0, L_hi=10.0)   # 6 480: 1 080 copies of every (T, D)
_GMIR = dict(nT=6, nLu=11, rL=3, nDu=24, rD=2, D_lo=-2.875, D_hi=2.875)   # 9 504: lateral samples +/- (0.125 + 0.25 k), exact negatives

# name -> parameters (filled in at the end of the module; tests/test_ladder_scenes.py asserts what the table is there for)
SCENES = {}
# scenes outside the table of the selection modules (build() finds them too): a longer horizon for the modules on sharded plans
EXTRA_SCENES = {}


@dataclasses.dataclass
class Scene:
    name: str
    spec: SceneSpec
    inputs: PlanInputs
    obstacles: ObstacleTables
    ref: tuple                # s, theta, curvature, curvature rate, xy

    @property
    def n_candidates(self):
        return self.inputs.n_candidates

    def setup(self, ctx):
        ctx.set_reference(*self.ref, 20.0)
        ctx.set_obstacles(self.obstacles)

    def oracle_tables(self):
        from oracle import oracle
        return oracle.OracleTables(*self.ref, 20.0, self.obstacles)

    def triple_ids(self):
        """per candidate: number of its (T, L, D) VALUE triple -- duplicates share one"""
        sp = self.spec
        iT, iL, iD = np.meshgrid(np.arange(sp.nT) % 2, np.arange(sp.nLu * sp.rL) % sp.nLu, np.arange(sp.nDu * sp.rD) % sp.nDu, indexing="ij")
        return ((iT * sp.nLu + iL) * sp.nDu + iD).ravel()


def build(name) -> Scene:
    sp = SCENES[name] if name in SCENES else EXTRA_SCENES[name]
    s = np.arange(0.0, 201.0, 1.0)
    z = np.zeros_like(s)
    T = np.array([2.0, 1.6] * (sp.nT // 2))
    L = np.tile(np.linspace(sp.L_lo, sp.L_hi, sp.nLu), sp.rL)
    D = np.tile(np.linspace(sp.D_lo, sp.D_hi, sp.nDu), sp.rD)
    veh = dict(W.VEHICLE2)
    if sp.a_max is not None:
        veh["a_max"] = sp.a_max
    p = make_params(dt=DT, N=sp.n_steps, factor=1, time_step0=0, low_vel_mode=False, lon_mode=0, flags=0, x0_lon=[10.0, 10.0, 0.0],
                    x0_lat=[0.0, 0.0, 0.0], x0_orientation=0.0, **veh)
    inp = PlanInputs(p, make_cost(desired_speed=10.0), T, W.traj_len_of(T, DT), L, D)
    wall = ObstacleTables(static_obb=[[sp.x_near + 9.0, sp.off, 0.0, 9.0, sp.w]])
    return Scene(name, sp, inp, wall, (s, z, z, z, np.stack((s, z), 1)))


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(scene, oracle result) -- computed once per process and left unchanged"""
    from oracle import oracle
    sc = build(name)
    run = oracle.plan(sc.inputs, sc.oracle_tables(), want_states=False, nthreads=8)
    run.status.setflags(write=False)
    run.cost.setflags(write=False)
    return sc, run


# ---- the selection, in plain NumPy ------------------------------------------------------------------------------------------------
def sort_order(cost):
    """indices (local) of the candidates that have a cost, in ascending (cost, index) order"""
    have = np.flatnonzero(~np.isnan(cost))
    return have[np.lexsort((have, cost[have]))]


def reference_selection(cost, labels, lo=0):
    """(winner index (global, -1: none), winner cost (NaN: none), colliding candidates ahead of the winner): the lexicographic
    (cost, index) minimum over the free candidates (label 1 with a cost) and the number of colliding ones (label 3) that sort
    before it -- all of them without a winner.  ``cost`` / ``labels``: local arrays of the candidates lo, lo + 1, ..."""
    cost = np.asarray(cost, dtype=np.float64)
    labels = np.asarray(labels)
    free = np.flatnonzero((labels == 1) & ~np.isnan(cost))
    coll = np.flatnonzero(labels == 3)
    if len(free) == 0:
        return -1, float("nan"), int(len(coll))
    wc = cost[free].min()
    wi = int(free[cost[free] == wc][0])
    before = int(np.count_nonzero((cost[coll] < wc) | ((cost[coll] == wc) & (coll < wi))))
    return lo + wi, float(wc), before


def reason_counts(status):
    """rp_result.reason_counts of a batch with these status words: candidates per first-failure reason 1 .. 7 (slot 0 stays 0)"""
    r = np.bincount((np.asarray(status) >> 4) & 7, minlength=8).astype(np.int64)
    r[0] = 0
    return r


def count_before(cost, labels, key_cost, key_index, lo=0):
    """colliding candidates (label 3) that sort before the key (cost, global index)"""
    coll = np.flatnonzero(np.asarray(labels) == 3)
    c = np.asarray(cost)[coll]
    return int(np.count_nonzero((c < key_cost) | ((c == key_cost) & (lo + coll < key_index))))


def rank_of_winner(cost, labels):
    """feasible candidates (labels 1 and 3) ahead of the winner in (cost, index) order; None without a winner"""
    wi, wc, _ = reference_selection(cost, labels)
    if wi < 0:
        return None
    feas = np.flatnonzero((labels == 1) | (labels == 3))
    c = cost[feas]
    return int(np.count_nonzero((c < wc) | ((c == wc) & (feas < wi))))


def tie_groups(cost, labels):
    """list of index arrays: the groups of feasible candidates whose costs are bit-equal, cheapest first"""
    feas = np.flatnonzero(((labels == 1) | (labels == 3)) & ~np.isnan(cost))
    if len(feas) == 0:
        return []
    bits = cost[feas].view(np.uint64)
    order = np.lexsort((feas, cost[feas]))
    f, b = feas[order], bits[order]
    cut = np.flatnonzero(b[1:] != b[:-1]) + 1
    return np.split(f, cut)


# ---- the cost-ordered stage, restated on the host ----------------------------------------------------------------------------------
def cost_key(c):
    b = np.asarray(c, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def lazy_bin(d):
    d = np.asarray(d, dtype=np.uint64)
    out = d.astype(np.int64)
    big = d >= 16
    if big.any():
        db = d[big]
        msb = np.zeros(len(db), dtype=np.int64)
        t = db.copy()
        for sh in (32, 16, 8, 4, 2, 1):
            m = (t >> np.uint64(sh)) != 0
            msb[m] += sh
            t[m] >>= np.uint64(sh)
        out[big] = (msb - 3) * 16 + ((db >> (msb - 4).astype(np.uint64)) & np.uint64(15)).astype(np.int64)
    return out


@dataclasses.dataclass
class StageModel:
    n_feasible: int
    sizes: tuple          # candidates of the three lists (uncapped)
    overflow: int         # bit l: list l over its capacity
    ran: tuple            # the rounds run_lazy runs (an empty second or third list is passed over)
    path: int             # 1: a round delivered the result, 2: the eager kernel (or the sweep) has to
    winner: int           # global index the stage itself delivers (path 1), else None
    m: int                # summed sizes of the lists of the rounds that ran (path 1)
    labelled: np.ndarray  # local indices of the colliding candidates the rounds label (path 1)


def stage_model(cost, labels, lo=0) -> StageModel:
    """What the list rounds do with a batch of these costs and (eager) labels: lists = the feasible candidates whose histogram
    bin is at most the first bin at which the cumulative count reaches 128 / 1 024 / 8 192; round l runs list l; a round with a
    free candidate, or after which every feasible candidate has been looked at, ends the stage (path 1); an over-full list among
    those run so far, or three rounds without a free candidate, leave the plan to the eager kernel or the sweep (path 2)."""
    feas = np.flatnonzero(((labels == 1) | (labels == 3)) & ~np.isnan(cost))
    nf = len(feas)
    none = np.zeros(0, dtype=np.int64)
    if nf == 0:   # (key_min 0, all edges 0: empty lists; round 0 finds checked 0 >= feasible 0)
        return StageModel(0, (0, 0, 0), 0, (0,), 1, -1, 0, none)
    key = cost_key(cost[feas])
    bins = lazy_bin(key - key.min())
    cum = np.cumsum(np.bincount(bins, minlength=1024))
    top, prev, sizes, ov = [], 0, [], 0
    for l in range(3):
        at = np.flatnonzero(cum >= LIST_TARGET[l])
        b = int(at[0]) if len(at) else 1023
        top.append(b)
        sizes.append(int(cum[b]) - prev)
        prev = int(cum[b])
        if sizes[-1] > LIST_CAP[l]:
            ov |= 1 << l
    checked = m = 0
    lab_parts, ran = [], []
    for l in range(3):
        if l > 0 and sizes[l] == 0:
            continue
        ran.append(l)
        lst = feas[(bins <= top[l]) & (bins > (top[l - 1] if l else -1))]
        if ov & ((2 << l) - 1):
            return StageModel(nf, tuple(sizes), ov, tuple(ran), 2, None, 0, none)
        m += len(lst)
        lab_parts.append(lst[labels[lst] == 3])
        free = lst[labels[lst] == 1]
        if len(free):
            wc = cost[free].min()
            return StageModel(nf, tuple(sizes), ov, tuple(ran), 1, lo + int(free[cost[free] == wc][0]), m, np.concatenate(lab_parts))
        checked += len(lst)
        if checked >= nf:
            return StageModel(nf, tuple(sizes), ov, tuple(ran), 1, -1, m, np.concatenate(lab_parts))
    return StageModel(nf, tuple(sizes), ov, tuple(ran), 2, None, 0, none)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
_scene = SceneSpec

SCENES.update({
    # -- the winner's rank on the small grid: first list, second list, third list
    "rank0_far_ties": _scene(**_G8, w=1.0, x_near=34.0),       # wall out of reach: the winner is the cheapest candidate, its copies 6 489 apart
    "rank72": _scene(**_G8, w=1.0, x_near=33.5),
    "rank504": _scene(**_G8, w=1.0, x_near=33.0),
    "rank936": _scene(**_G8, w=0.05),
    "rank1584": _scene(**_G8, w=0.4),
    "rank3654": _scene(**_G8, w=1.5),
    # -- beyond the one-workgroup epilogue: third list, just behind the lists (10 768 candidates), beyond their capacity
    "g48_rank6528": _scene(**_G48, w=0.3),
    "g48_rank10080": _scene(**_G48, w=0.5),
    "g48_rank12000": _scene(**_G48, w=0.7),
    "g48_rank24080": _scene(**_G48, w=1.5),
    "g135_rank29808": _scene(**_G135, w=0.6),
    # -- 131 072 candidates whose T copies lie exactly 65 536 apart: with four candidates per workgroup (one-wavefront workgroups, 64 lanes
    #    per candidate) the partials of the winner and of a free copy of it reach the SAME lane of rp_fold_partials_kernel, 16 384 apart
    "fold_alias": _scene(nT=4, nLu=32, rL=4, nDu=32, rD=8, w=0.3),
    # -- every feasible candidate collides: 44, 4 248 and 24 880 of them
    "all_collide_44": _scene(nT=2, nLu=3, rL=2, nDu=5, rD=2, w=6.0),
    "all_collide_4248": _scene(**_G8, w=2.5),
    "all_collide_24880": _scene(**_G48, w=2.0),
    # -- no feasible candidate (an acceleration limit nothing satisfies); cheapest cost exactly 0.0 (L = 10 and D = 0 are samples)
    "none_feasible": _scene(**_G8, w=1.0, a_max=1e-6),
    "zero_cost": _scene(nT=6, nLu=11, rL=3, nDu=21, rD=2, w=0.05, L_lo=10.0, D_lo=0.0),
    # -- more than a first list of copies of the cheapest cost: the group free / colliding with a free group behind it
    "overflow_free": _scene(**_GOV, w=1.0, x_near=34.0),
    "overflow_blocked": _scene(**_GOV, D_lo=-1.5, D_hi=1.2, w=1.0, off=-1.0),
    # -- symmetric lateral grid, wall on the negative side: candidates at -d collide, their twins at +d are free
    "mirror_rank73": _scene(**_GMIR, w=0.5, off=-1.0),
    "mirror_rank721": _scene(**_GMIR, w=1.0, off=-1.0),
})
# -- N = 40 (41 steps: three step blocks of 16, two of 32, one of 64 lanes -- the horizons of 33 .. 64 steps have their own thresholds
#    between the lanes per candidate): the small grid, the winner behind the first list
EXTRA_SCENES.update({
    "n40_g8": _scene(**_G8, w=0.4, n_steps=40),
})
N40 = "n40_g8"
LARGEST = "g135_rank29808"
FOLD_ALIAS = "fold_alias"
MIRROR = ("mirror_rank73", "mirror_rank721")
