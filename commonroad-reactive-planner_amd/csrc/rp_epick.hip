// rp_epick.hip -- librp_epick.so: the pick under a risk bound of include/rp_epick.h (MI355X / gfx950).
//
// K given curvilinear trajectories x n poses along ONE reference path, against the static shapes and M sampled predictions
// ("members") of the dynamic obstacles: the lift of rp_lift.h, the cost of rp_pick.h, the collision tests of rp_check.h per member,
// the members' weights summed per trajectory and the cheapest kinematically feasible trajectory under the bound, with the poses and
// the hit flags staying on the device between the stages.  The mapping is the family's: a lane is a pose, a wavefront 64 consecutive
// poses of one trajectory, a workgroup four wavefronts.  Nothing the siblings state is restated: the per-pose lift step
// (rp_lift_rules.h with rp_lift_walk.inc), the obstacle walk (rp_check_rules.h) and the cost (rp_pick_cost.h) come from the files they
// are stated in once.  What is written here is the member dimension, the risk, the final stage and the host side.
//
//   rp_epick_lift_kernel      one wavefront walks one trajectory: eight planes (x, y, theta always, the rest where asked for), the
//                             kinematic verdict and the cost
//   rp_epick_collide_kernel   (trajectory, chunk) wavefronts x member blocks over the kept poses; a trajectory that is not feasible
//                             returns at once; the static shapes once per wavefront, then member by member
//   rp_epick_risk_kernel      64 trajectories per workgroup: "none" -> -1, members_hit, risk in ascending m, the label and its step
//   rp_epick_final_kernel     one workgroup: the winner, the counts
//   rp_epick_lift_kernel      once more, one wavefront on the winner alone: its state block
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_check_rules.h"   // the obstacle tables and their builder, cc.collide and both tests of a chunk: shared with rp_check.hip and rp_pick.hip
#include "rp_lift_rules.h"    // the segment row, the segment search, the step's checks: shared with rp_lift.hip and rp_pick.hip
#include "rp_pick_cost.h"     // the cost's scalars and the terms of a pose: shared with rp_pick.hip
#include "rp_session.h"       // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_epick.h"

namespace {

constexpr int EP_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int EP_WAVES = EP_BLOCK / 64;
constexpr int EP_LF_LDS_ROWS = 384;             // most segment rows staged in LDS: the lift's capacity (LF_LDS_ROWS of rp_lift.hip)
constexpr int EP_CK_LDS_ROWS = 128;             // most static rows staged in LDS: the checker's capacity (CK_LDS_ROWS of rp_check.hip)
// Members one wavefront walks, one after the other (the member blocks are the grid's y dimension).  A larger block shares the ego
// rectangles and the static test of a wavefront among more members, a smaller one puts more wavefronts on the device.  The walk of a
// member is ck_pose_hit / ck_segment_hit unchanged, so the loads of two members do not overlap as they do in rp_ensemble.hip
// (profiles/probe_epick.py on libraries built with -DEP_MEMBER_BLOCK_PROBE=<n>; profiles/epick_batch.txt).
#ifdef EP_MEMBER_BLOCK_PROBE
constexpr int EP_MEMBER_BLOCK = EP_MEMBER_BLOCK_PROBE;
#else
constexpr int EP_MEMBER_BLOCK = 4;
#endif
constexpr int EP_RISK_BLOCK = 1024;             // risk kernel: sixteen wavefronts, 64 trajectories per workgroup
constexpr int EP_RISK_PER_WAVE = 64 / (EP_RISK_BLOCK / 64);
constexpr int EP_FINAL_BLOCK = 1024;            // the one workgroup of rp_epick_final_kernel
constexpr unsigned long long EP_NO_K = ~0ull;

static_assert(EP_MEMBER_BLOCK >= 1, "a wavefront walks at least one member");

// the scalars of a call on the device, 16 words
enum { RED_BEST, RED_COST, RED_FEASIBLE, RED_COLLISION, RED_BEFORE, RED_REASON0 /* .. + 7 */, RED_BEST_HIT = RED_REASON0 + 8, RED_BEST_RISK, RED_WORDS = 16 };

// the row of a state block each of the eight planes and each of the six input planes is
constexpr int EP_PLANE_ROW[LF_PLANES] = {RP_X, RP_Y, RP_THETA, RP_V, RP_A, RP_KAPPA, RP_KAPPA_DOT, RP_THETA_CL};
constexpr int EP_INPUT_ROW[6] = {RP_S, RP_S_DOT, RP_S_DDOT, RP_D, RP_D_DOT, RP_D_DDOT};

// where a launch writes each of the eight planes (nullptr: nowhere)
struct EpPlanes {
    double *plane[LF_PLANES];
};

// the members on the device: planes [M][7][n_dyn][n_steps] -- member m's are a CkTables' dyn -- and weight [M]
struct EpMembers {
    const double *dyn;
    const double *weight;
    int32_t n_members, n_dyn, n_steps, dyn_t0;
};

// Wavefront w of the grid = trajectory w, as rp_pick_lift_kernel: the walk of rp_lift_walk.inc, the planes the launch has a place for
// at [k][i], the cost's terms of the lane's poses in ascending order and the 64 partial sums in a fixed butterfly.  in: the six input
// planes, each [K][n].  With `sel` the launch is one workgroup whose first wavefront lifts trajectory sel[0] alone into a state block
// (`block`, [RP_N_ARRAYS][n]; the planes point at its rows): the same code on the same inputs, so the rows are bit-equal to the planes
// of the launch over all K.  sel[0] beyond K: no winner, the block is NaN.
template <bool LDS>
__global__ __launch_bounds__(EP_BLOCK) void rp_epick_lift_kernel(LfTable tb, LfKin kin, PkCost cc, const double *in, const int32_t *len, const double *theta0,
                                                                 long long K, int n, const unsigned long long *sel, double *block, EpPlanes out,
                                                                 uint32_t *status, double *cost) {
    extern __shared__ double sh_rows[];     // n_seg rows (the launch sizes it); none if !LDS
    if (LDS) {
        const int nd = tb.n_seg * LF_ROW;   // <= EP_LF_LDS_ROWS * LF_ROW: the host picks this variant and allocates nd doubles
        for (int q = threadIdx.x; q < nd; q += EP_BLOCK) sh_rows[q] = tb.rows[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    long long k = (long long)blockIdx.x * EP_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    size_t obase;
    if (sel) {                              // (wave-uniform, behind the only barrier)
        if (k != 0) return;
        const unsigned long long kk = sel[0];
        if (kk >= (unsigned long long)K) {
            for (int q = lane; q < RP_N_ARRAYS * n; q += 64) block[q] = __builtin_nan("");
            return;
        }
        k = (long long)kk;
        obase = 0;
    } else {
        if (k >= K) return;                 // (a whole wavefront)
        obase = (size_t)k * (size_t)n;
    }
    const LfRows<LDS> row = {sh_rows, tb.rows};
    const size_t P = (size_t)K * (size_t)n, base = (size_t)k * (size_t)n;
    const int L = len ? len[k] : n;         // 1 <= L <= n, checked by the host
    const int last = L - 1, mid = L / 2;
    double sum = 0.0;
    const PkAddCost add_cost = {cc, sum, last, mid};
    // the walk itself is text shared with rp_lift.hip; here a pose goes to the planes this launch has a place for, and into the cost
#define LF_PUT_NAN(I)                            \
    _Pragma("unroll") for (int pl = 0; pl < LF_PLANES; ++pl) \
        if (out.plane[pl]) out.plane[pl][obase + (I)] = nan
#define LF_PUT_POSE(I, X, Y, TH, V, A, KP, KPD, THCL, LIVE, S, D)                  \
    {                                                                               \
        const double pose[LF_PLANES] = {X, Y, TH, V, A, KP, KPD, THCL};             \
        _Pragma("unroll") for (int pl = 0; pl < LF_PLANES; ++pl)                    \
            if (out.plane[pl]) out.plane[pl][obase + (I)] = pose[pl];               \
        if (LIVE) add_cost(I, pose[3], pose[4], pose[7], S, D);                     \
    }
#include "rp_lift_walk.inc"
#undef LF_PUT_NAN
#undef LF_PUT_POSE
    const uint32_t st = lf_verdict(best);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (status && lane == 0) {
        status[k] = st;
        cost[k] = st == RP_LABEL_FEASIBLE ? sum : nan;
    }
    if (sel) {                              // the block's six input rows, NaN behind the trajectory's end
        for (int i = lane; i < n; i += 64)
#pragma unroll
            for (int q = 0; q < 6; ++q) block[(size_t)EP_INPUT_ROW[q] * (size_t)n + i] = i < L ? in[(size_t)q * P + base + i] : nan;
    }
}

// Wavefront w of the grid's x dimension = chunk w % nchunk of trajectory w / nchunk, blockIdx.y = block of EP_MEMBER_BLOCK members; a
// trajectory whose verdict is not RP_LABEL_FEASIBLE returns at once.  Each test first against the static shapes alone (stat: a
// CkTables without dynamic rows) -- their first hit of the wavefront, a ballot, holds in every member -- then, member by member, the
// lanes IN FRONT of that hit against a CkTables that holds nothing but the member's planes (a lane behind the static hit cannot lower
// the first hit).  poses: planes x | y | theta, each [K][n].  first_pose / first_seg ([K][M]) hold CK_NONE on entry (a fill in front
// of the launch) and receive the smallest colliding index by one atomicMin per (wavefront, member) that has a hit.
template <bool LDS>
__global__ __launch_bounds__(EP_BLOCK) void rp_epick_collide_kernel(CkTables stat, EpMembers mb, const double *poses, const int32_t *len, const uint32_t *status,
                                                                    int K, int n, int nchunk, uint32_t mode, double wb_rear_axle, double hl, double hw, int t0,
                                                                    int factor, int32_t *first_pose, int32_t *first_seg) {
    __shared__ double sh_rows[LDS ? EP_CK_LDS_ROWS * CK_ROW : 1];
    if (LDS) {
        const int nd = (stat.n_sobb + stat.n_tri + stat.n_circ) * CK_ROW;   // <= EP_CK_LDS_ROWS * CK_ROW: the host picks this variant
        for (int q = threadIdx.x; q < nd; q += EP_BLOCK) sh_rows[q] = stat.stat[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * EP_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= (long long)K * nchunk) return;   // (a whole wavefront, behind the only barrier)
    const int k = (int)(w / nchunk), chunk = (int)(w % nchunk);
    if (status[k] != RP_LABEL_FEASIBLE) return;   // wave-uniform: not kinematically feasible, not tested
    const int M = mb.n_members;
    const int m_begin = (int)blockIdx.y * EP_MEMBER_BLOCK;
    const int m_end = m_begin + EP_MEMBER_BLOCK < M ? m_begin + EP_MEMBER_BLOCK : M;
    const int i = chunk * 64 + lane;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    const bool have = i < L;
    const size_t plane = (size_t)K * (size_t)n;
    const size_t at = (size_t)k * (size_t)n + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never asked
    const Obb ego = ck_ego(poses, plane, at, wb_rear_axle, hl, hw);
    const size_t member = (size_t)7 * (size_t)mb.n_dyn * (size_t)mb.n_steps;   // doubles of one member's planes
    // member m alone: no static shapes, its own dynamic rows
    auto tables_of = [&](int m) -> CkTables { return {nullptr, mb.dyn + (size_t)m * member, 0, 0, 0, mb.n_dyn, mb.n_steps, mb.dyn_t0}; };
    // the member's first hit of this wavefront: its own in front of the static one, else the static one
    auto record = [&](int32_t *first, int m, bool hit, int sfirst) {
        const unsigned long long b = __ballot(hit);
        const int f = b != 0 ? __ffsll(b) - 1 : sfirst;
        if (f < 64 && lane == 0) atomicMin(&first[(size_t)k * (size_t)M + (size_t)m], chunk * 64 + f);
    };
    if (mode & RP_TRAJ_POSES) {
        const unsigned long long bs = __ballot(ck_pose_hit<LDS>(stat, sh_rows, ego, hl, hw, t0, factor, i, have));
        const int sfirst = bs != 0 ? __ffsll(bs) - 1 : 64;
#pragma unroll 1
        for (int m = m_begin; m < m_end; ++m)   // wave-uniform
            record(first_pose, m, ck_pose_hit<LDS>(tables_of(m), sh_rows, ego, hl, hw, t0, factor, i, have && lane < sfirst), sfirst);
    }
    if (mode & RP_TRAJ_SWEPT) {
        const unsigned long long bs = __ballot(ck_segment_hit<LDS>(stat, sh_rows, ego, poses, plane, at, wb_rear_axle, hl, hw, t0, i, L, lane));
        const int sfirst = bs != 0 ? __ffsll(bs) - 1 : 64;
        // the segments in front of the static hit are those of a trajectory that ends with the pose the hit segment starts at
        const int front = chunk * 64 + sfirst + 1, Lm = front < L ? front : L;
#pragma unroll 1
        for (int m = m_begin; m < m_end; ++m)   // wave-uniform
            record(first_seg, m, ck_segment_hit<LDS>(tables_of(m), sh_rows, ego, poses, plane, at, wb_rear_axle, hl, hw, t0, i, Lm, lane), sfirst);
    }
}

// A workgroup is 64 trajectories.  Members go by in tiles of 64: each wavefront takes EP_RISK_PER_WAVE trajectories with its lanes
// across the tile's members -- CK_NONE -> -1 in the first-hit matrices of the requested tests, the smallest pose and segment hit over
// the members, and the tile's hit flags of a trajectory as one 64-bit ballot into LDS, trajectory after trajectory, so that the lanes
// of the first wavefront, one per trajectory, read consecutive words.  Those lanes walk the flags in ascending m: members_hit counts
// them, risk adds their weights in double, one after the other, from 0.0 -- the order of include/rp_epick.h.  Then the label: a
// kinematically feasible trajectory over the bound becomes RP_LABEL_INFEASIBLE_COLLISION with its step.  mode == 0: no matrix is read,
// every count is 0 and every risk 0.0.
__global__ __launch_bounds__(EP_RISK_BLOCK) void rp_epick_risk_kernel(int K, int M, uint32_t mode, double max_risk, const double *weight, uint32_t *status,
                                                                      int32_t *first_pose, int32_t *first_seg, int32_t *members_hit, double *risk) {
    __shared__ unsigned long long sh_flags[64];
    __shared__ int32_t sh_pose[64], sh_seg[64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int32_t min_pose[EP_RISK_PER_WAVE], min_seg[EP_RISK_PER_WAVE];   // the lane's own, over the members it saw
#pragma unroll
    for (int q = 0; q < EP_RISK_PER_WAVE; ++q) min_pose[q] = min_seg[q] = CK_NONE;
    int count = 0;         // first wavefront: of trajectory blockIdx.x * 64 + lane
    double sum = 0.0;
    const int tiles = mode != 0 ? (M + 63) / 64 : 0;
#pragma unroll 1
    for (int tile = 0; tile < tiles; ++tile) {   // uniform over the workgroup
        const int m = tile * 64 + lane;
#pragma unroll
        for (int q = 0; q < EP_RISK_PER_WAVE; ++q) {
            const int slot = wave * EP_RISK_PER_WAVE + q;
            const long long k = (long long)blockIdx.x * 64 + slot;   // wave-uniform
            bool hit = false;
            if (k < K && m < M) {
                const size_t at = (size_t)k * (size_t)M + (size_t)m;
                if (mode & RP_TRAJ_POSES) {
                    const int32_t f = first_pose[at];
                    if (f >= CK_NONE) first_pose[at] = -1;
                    else { hit = true; min_pose[q] = f < min_pose[q] ? f : min_pose[q]; }
                }
                if (mode & RP_TRAJ_SWEPT) {
                    const int32_t f = first_seg[at];
                    if (f >= CK_NONE) first_seg[at] = -1;
                    else { hit = true; min_seg[q] = f < min_seg[q] ? f : min_seg[q]; }
                }
            }
            const unsigned long long b = __ballot(hit);
            if (lane == 0) sh_flags[slot] = b;
        }
        __syncthreads();
        if (wave == 0) {
            const unsigned long long flags = sh_flags[lane];
            const int members = M - tile * 64 < 64 ? M - tile * 64 : 64;
#pragma unroll 1
            for (int j = 0; j < members; ++j) {   // ascending m
                const double wj = weight[tile * 64 + j];   // (the same address in every lane)
                if ((flags >> j) & 1ull) { ++count; sum += wj; }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < EP_RISK_PER_WAVE; ++q) {
        int32_t fp = min_pose[q], fs = min_seg[q];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int32_t op = __shfl_xor(fp, o), os = __shfl_xor(fs, o);
            fp = op < fp ? op : fp;
            fs = os < fs ? os : fs;
        }
        if (lane == 0) { sh_pose[wave * EP_RISK_PER_WAVE + q] = fp; sh_seg[wave * EP_RISK_PER_WAVE + q] = fs; }
    }
    __syncthreads();
    if (wave != 0) return;
    const long long k = (long long)blockIdx.x * 64 + lane;
    if (k >= K) return;
    if (status[k] != RP_LABEL_FEASIBLE) {   // not tested: its rows held nothing but CK_NONE
        members_hit[k] = 0;
        risk[k] = 0.0;
        return;
    }
    members_hit[k] = count;
    risk[k] = sum;
    if (sum > max_risk) {                   // (then some member has a hit)
        const int32_t fp = sh_pose[lane], fs = sh_seg[lane];
        uint32_t step = (uint32_t)(fp < CK_NONE ? fp : fs);
        step = step > 0xFFFu ? 0xFFFu : step;
        status[k] = RP_LABEL_INFEASIBLE_COLLISION | (step << 8);
    }
}

// The scalars of a call, by ONE workgroup that strides over the K trajectories as rp_pick_final_kernel does (no atomics, nothing to
// initialise, the same result whatever K); the labels are rp_epick_risk_kernel's.  First pass: the lexicographic minimum of (cost, k)
// over the trajectories left feasible and the counts.  Second pass: the trajectories over the bound with (cost, k) below the
// winner's -- all of them when there is none.
__global__ __launch_bounds__(EP_FINAL_BLOCK) void rp_epick_final_kernel(long long K, uint32_t mode, const uint32_t *status, const double *cost,
                                                                        const int32_t *members_hit, const double *risk, unsigned long long *red) {
    constexpr int NW = EP_FINAL_BLOCK / 64;
    __shared__ unsigned long long sh_k[NW];
    __shared__ double sh_c[NW];
    __shared__ uint32_t sh_cnt[NW][9];   // (K <= RP_EPICK_MAX_POSES = 2^24: a count fits)
    __shared__ uint32_t sh_before[NW];
    unsigned long long bestk = EP_NO_K;
    double bestc = 0.0;
    uint32_t cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // cnt[0]: kinematically feasible, cnt[8]: of them over the bound
#pragma unroll 1
    for (long long k = threadIdx.x; k < K; k += EP_FINAL_BLOCK) {   // ascending: a thread keeps the first of equal costs
        const uint32_t st = status[k];
        const uint32_t label = RP_STATUS_LABEL(st);
        if (label == RP_LABEL_FEASIBLE) {
            ++cnt[0];
            const double cv = cost[k];
            if (cv == cv && (bestk == EP_NO_K || cv < bestc)) { bestc = cv; bestk = (unsigned long long)k; }
        } else if (label == RP_LABEL_INFEASIBLE_COLLISION) {
            ++cnt[0];
            ++cnt[8];
        } else {
            const uint32_t r = RP_STATUS_REASON(st);
#pragma unroll
            for (uint32_t q = 1; q < 8; ++q) cnt[q] += r == q ? 1u : 0u;
        }
    }
    auto merge = [&](unsigned long long ok, double oc) {
        if (ok != EP_NO_K && (bestk == EP_NO_K || oc < bestc || (oc == bestc && ok < bestk))) { bestc = oc; bestk = ok; }
    };
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long ok = __shfl_xor(bestk, off);
        const double oc = __shfl_xor(bestc, off);
        merge(ok, oc);
#pragma unroll
        for (int q = 0; q < 9; ++q) cnt[q] += __shfl_xor(cnt[q], off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_k[wave] = bestk; sh_c[wave] = bestc;
#pragma unroll
        for (int q = 0; q < 9; ++q) sh_cnt[wave][q] = cnt[q];
    }
    __syncthreads();
    // every thread folds the 16 wavefronts' candidates in the same order: the same winner in each of them
    bestk = sh_k[0]; bestc = sh_c[0];
#pragma unroll 1
    for (int w = 1; w < NW; ++w) merge(sh_k[w], sh_c[w]);
    uint32_t before = 0;
    if (mode != 0) {
#pragma unroll 1
        for (long long k = threadIdx.x; k < K; k += EP_FINAL_BLOCK) {
            if (RP_STATUS_LABEL(status[k]) != RP_LABEL_INFEASIBLE_COLLISION) continue;
            const double cv = cost[k];
            before += (bestk == EP_NO_K || cv < bestc || (cv == bestc && (unsigned long long)k < bestk)) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off);
    if ((threadIdx.x & 63) == 0) sh_before[wave] = before;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int w = 1; w < NW; ++w) {
            before += sh_before[w];
#pragma unroll
            for (int q = 0; q < 9; ++q) cnt[q] += sh_cnt[w][q];
        }
        red[RED_BEST] = bestk;
        red[RED_COST] = (unsigned long long)__double_as_longlong(bestc);
        red[RED_FEASIBLE] = cnt[0];
        red[RED_COLLISION] = cnt[8];
        red[RED_BEFORE] = before;
        red[RED_REASON0] = 0ull;
#pragma unroll
        for (int q = 1; q < 8; ++q) red[RED_REASON0 + q] = cnt[q];
        const bool any = bestk != EP_NO_K;
        red[RED_BEST_HIT] = any ? (unsigned long long)members_hit[bestk] : 0ull;
        red[RED_BEST_RISK] = any ? (unsigned long long)__double_as_longlong(risk[bestk]) : 0ull;
    }
}

}  // namespace

struct rp_epick : RpSession {
    LfTable tb = {nullptr, 0, 0, 0.0, 0.0, 0.0};
    CkTables stat = {nullptr, nullptr, 0, 0, 0, 0, 0, 0};   // the static shapes alone: no dynamic rows
    EpMembers mb = {nullptr, nullptr, 1, 0, 0, 0};          // one member without dynamic obstacles; its weight (1.0) comes with create
    RpTable d_rows, d_stat, d_dyn, d_weight;
};

extern "C" {

int rp_epick_abi_version(void) { return RP_EPICK_ABI_VERSION; }

int rp_epick_create(rp_epick **out, int device) {
    int rc = session_create(out, device);
    if (rc != RP_OK) return rc;
    rp_epick *ep = *out;
    const std::vector<double> one(1, 1.0);   // the weight of the one member a fresh object has
    if ((rc = replace_tables(ep, {{&ep->d_weight, &one}})) != RP_OK) {
        (void)hipStreamDestroy(ep->stream);   // (without a stream the object has no device: every later call says so)
        ep->stream = nullptr;
        return rc;
    }
    ep->mb.weight = ep->d_weight.p;
    return RP_OK;
}

void rp_epick_destroy(rp_epick *ep) { session_destroy(ep); }

const char *rp_epick_last_error(const rp_epick *ep) { return session_last_error(ep, "null epick object"); }

int rp_epick_set_reference(rp_epick *ep, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta, const double *ref_curv,
                           const double *ref_curv_d, double proj_domain_d_limit) {
    if (!ep) return RP_EINVAL;
    if (!ep->stream) return fail(ep, RP_ESTATE, "rp_epick_set_reference: the object has no device (rp_epick_create failed)");
    std::vector<double> rows;
    std::string msg;
    int rc = lf_build_rows("rp_epick_set_reference", n, ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, proj_domain_d_limit, rows, msg);
    if (rc != RP_OK) return fail(ep, rc, msg);
    if ((rc = replace_tables(ep, {{&ep->d_rows, &rows}})) != RP_OK) return rc;
    ep->tb = {ep->d_rows.p, n - 1, lf_search_iters(n), ref_pos[0], ref_pos[n - 1], proj_domain_d_limit};
    return RP_OK;
}

int rp_epick_set_static(rp_epick *ep, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ) {
    if (!ep) return RP_EINVAL;
    if (!ep->stream) return fail(ep, RP_ESTATE, "rp_epick_set_static: the object has no device (rp_epick_create failed)");
    std::vector<double> a, none;
    std::string msg;
    int rc = ot_build("rp_epick_set_static", n_sobb, sobb, n_tri, tri, n_circ, circ, 0, 0, nullptr, a, none, msg);
    if (rc != RP_OK) return fail(ep, rc, msg);
    if ((rc = replace_tables(ep, {{&ep->d_stat, &a}})) != RP_OK) return rc;
    ep->stat = {ep->d_stat.p, nullptr, n_sobb, n_tri, n_circ, 0, 0, 0};
    return RP_OK;
}

int rp_epick_set_members(rp_epick *ep, int32_t n_members, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn, const double *weight) {
    if (!ep) return RP_EINVAL;
    if (!ep->stream) return fail(ep, RP_ESTATE, "rp_epick_set_members: the object has no device (rp_epick_create failed)");
    if (n_members < 1 || n_members > RP_EPICK_MAX_MEMBERS) return fail(ep, RP_EINVAL, "rp_epick_set_members: n_members outside 1 .. RP_EPICK_MAX_MEMBERS");
    if (n_dyn < 0 || n_steps < 0) return fail(ep, RP_EINVAL, "rp_epick_set_members: negative count");
    const int64_t plane64 = (int64_t)n_dyn * (int64_t)n_steps;   // < 2^62
    if (plane64 > RP_EPICK_MAX_DYN_ROWS || (int64_t)n_members * plane64 > RP_EPICK_MAX_DYN_ROWS)
        return fail(ep, RP_EINVAL, "rp_epick_set_members: n_members * n_dyn * n_steps beyond RP_EPICK_MAX_DYN_ROWS");
    if (plane64 && !dyn) return fail(ep, RP_EINVAL, "rp_epick_set_members: null table");
    if (weight)
        for (int32_t m = 0; m < n_members; ++m)
            if (!(weight[m] >= 0.0) || !std::isfinite(weight[m]))
                return fail(ep, RP_EINVAL, "rp_epick_set_members: weight[" + std::to_string(m) + "] is negative or not finite");
    // member by member the planes of rp_obstacle_tables.h: each member's part is a table ck_collides reads
    const size_t plane = (size_t)plane64;
    std::vector<double> all, w;
    try {
        all.assign((size_t)n_members * 7 * plane, 0.0);
        w.assign((size_t)n_members, 1.0);
    } catch (const std::bad_alloc &) {
        return fail(ep, RP_ENOMEM, "rp_epick_set_members: host memory");
    }
    if (weight) std::memcpy(w.data(), weight, (size_t)n_members * sizeof(double));
    for (size_t m = 0; m < (size_t)n_members; ++m) ot_dynamic_planes(all.data() + m * 7 * plane, plane, dyn + 5 * m * plane);
    const int rc = replace_tables(ep, {{&ep->d_dyn, &all}, {&ep->d_weight, &w}});
    if (rc != RP_OK) return rc;
    ep->mb = {ep->d_dyn.p, ep->d_weight.p, n_members, plane ? n_dyn : 0, plane ? n_steps : 0, dyn_t0};
    return RP_OK;
}

int rp_epick_select(rp_epick *ep, const rp_params *p, const rp_cost *cost, uint32_t mode, double max_risk, int64_t K, int32_t n_poses, const double *s,
                    const double *s_dot, const double *s_ddot, const double *d, const double *d_dot, const double *d_ddot, const int32_t *len,
                    const double *theta0, uint32_t flags, double *x, double *y, double *theta, double *v, double *a, double *kappa, double *kappa_dot,
                    double *theta_cl, uint32_t *status, double *cost_out, int32_t *members_hit, double *risk, int32_t *first_pose_hit,
                    int32_t *first_segment_hit, rp_epick_result *result, double *best_states) {
    if (!ep) return RP_EINVAL;
    if (!p || !cost) return fail(ep, RP_EINVAL, "rp_epick_select: null params or cost");
    if (p->struct_size != sizeof(rp_params)) return fail(ep, RP_EABI, "rp_epick_select: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (cost->struct_size != sizeof(rp_cost)) return fail(ep, RP_EABI, "rp_epick_select: rp_cost.struct_size is not this library's sizeof(rp_cost)");
    if (result && result->struct_size != sizeof(rp_epick_result))
        return fail(ep, RP_EABI, "rp_epick_select: rp_epick_result.struct_size is not this library's sizeof(rp_epick_result)");
    if ((mode & ~(RP_TRAJ_POSES | RP_TRAJ_SWEPT)) != 0) return fail(ep, RP_EINVAL, "rp_epick_select: mode has a bit besides RP_TRAJ_POSES and RP_TRAJ_SWEPT");
    if (!(max_risk >= 0.0)) return fail(ep, RP_EINVAL, "rp_epick_select: max_risk is NaN or negative");
    if (K < 0 || n_poses < 1) return fail(ep, RP_EINVAL, "rp_epick_select: K < 0 or n_poses < 1");
    if (K > RP_EPICK_MAX_POSES || K * (int64_t)n_poses > RP_EPICK_MAX_POSES) return fail(ep, RP_EINVAL, "rp_epick_select: K * n_poses beyond RP_EPICK_MAX_POSES");
    const int M = ep->mb.n_members;
    if (K * (int64_t)M > RP_EPICK_MAX_VERDICTS) return fail(ep, RP_EINVAL, "rp_epick_select: K * n_members beyond RP_EPICK_MAX_VERDICTS");
    if (flags != 0) return fail(ep, RP_EINVAL, "rp_epick_select: unknown flags");
    if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fail(ep, RP_EINVAL, "rp_epick_select: dt must be positive");
    if (cost->kind != RP_COST_DEFAULT && cost->kind != RP_COST_FAILSAFE)
        return fail(ep, RP_EINVAL, "rp_epick_select: cost kind must be RP_COST_DEFAULT or RP_COST_FAILSAFE");
    const double desired[3] = {cost->desired_speed, cost->desired_d, cost->desired_s};
    for (double q : desired)
        if (!std::isnan(q) && !std::isfinite(q)) return fail(ep, RP_EINVAL, "rp_epick_select: a desired value of the cost is infinite");
    if (!(mode & RP_TRAJ_POSES) && first_pose_hit) return fail(ep, RP_EINVAL, "rp_epick_select: first_pose_hit without RP_TRAJ_POSES");
    if (!(mode & RP_TRAJ_SWEPT) && first_segment_hit) return fail(ep, RP_EINVAL, "rp_epick_select: first_segment_hit without RP_TRAJ_SWEPT");
    const double *planes[6] = {s, s_dot, s_ddot, d, d_dot, d_ddot};
    if (K > 0)
        for (const double *q : planes)
            if (!q) return fail(ep, RP_EINVAL, "rp_epick_select: a null input plane");
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(ep, RP_EINVAL, "rp_epick_select: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (!ep->stream) return fail(ep, RP_ESTATE, "rp_epick_select: the object has no device (rp_epick_create failed)");
    if (!ep->tb.rows) return fail(ep, RP_ESTATE, "rp_epick_select: no reference set (rp_epick_set_reference)");
    const size_t nz = (size_t)n_poses, block_bytes = (size_t)RP_N_ARRAYS * nz * sizeof(double);
    if (K == 0) {
        if (result) {
            result->best = -1; result->best_cost = std::nan("");
            result->n_feasible = 0; result->n_collision = 0; result->n_collision_before_best = 0;
            std::memset(result->reason_counts, 0, sizeof(result->reason_counts));
            result->best_members_hit = -1; result->best_risk = std::nan("");
        }
        if (best_states)
            for (size_t q = 0; q < (size_t)RP_N_ARRAYS * nz; ++q) best_states[q] = std::nan("");
        return RP_OK;
    }
    RP_TRY(ep, hipSetDevice(ep->device));
    const size_t P = (size_t)K * nz, Kz = (size_t)K, V = Kz * (size_t)M, mat_bytes = V * sizeof(int32_t);
    // inputs: the six planes | theta0? [K] | len? [K]
    const size_t th0_off = 6 * P * sizeof(double), len_off = th0_off + (theta0 ? Kz * sizeof(double) : 0);
    const size_t in_bytes = len_off + (len ? Kz * sizeof(int32_t) : 0);
    // results on the device: scalars | the winner's block [RP_N_ARRAYS][n] | cost [K] | risk [K] | status [K] | members_hit [K] |
    // (8-byte aligned) first_pose [K][M] | first_seg [K][M] | (8-byte aligned) the eight planes in the order of the arguments.  A call
    // copies back the front of it as far as it asks for, each matrix it asks for, and of the planes the run from the first to the last
    // one it asks for; planes behind the last one that is written have no room.
    const size_t blk_off = RED_WORDS * sizeof(unsigned long long), cost_off = blk_off + block_bytes, risk_off = cost_off + Kz * sizeof(double);
    const size_t st_off = risk_off + Kz * sizeof(double), mh_off = st_off + Kz * sizeof(uint32_t), front_end = mh_off + Kz * sizeof(int32_t);
    const size_t fp_off = align8(front_end), fs_off = fp_off + mat_bytes, pl_off = align8(fs_off + mat_bytes);
    double *const outs[LF_PLANES] = {x, y, theta, v, a, kappa, kappa_dot, theta_cl};
    int pl_first = LF_PLANES, pl_end = 0;
    for (int q = 0; q < LF_PLANES; ++q)
        if (outs[q]) { pl_first = q < pl_first ? q : pl_first; pl_end = q + 1; }
    const int n_dev_planes = pl_end > 3 ? pl_end : 3;   // x, y, theta are kept for the collision test whoever asks
    const size_t dev_bytes = pl_off + (size_t)n_dev_planes * P * sizeof(double);
    const size_t front_bytes = members_hit ? front_end : status ? mh_off : risk ? st_off : cost_out ? risk_off : best_states ? cost_off : blk_off;
    const size_t pl_bytes = pl_end > pl_first ? (size_t)(pl_end - pl_first) * P * sizeof(double) : 0;
    // on the host: the front | (8-byte aligned) the matrices asked for | the planes asked for
    const size_t h_fp_off = align8(front_bytes), h_fs_off = h_fp_off + (first_pose_hit ? mat_bytes : 0);
    const size_t h_pl_off = align8(h_fs_off + (first_segment_hit ? mat_bytes : 0));
    const int rc = grow_call(ep, "rp_epick", in_bytes, h_pl_off + pl_bytes, dev_bytes);
    if (rc != RP_OK) return rc;
    char *h_in = static_cast<char *>(ep->h_in.p);
    const char *d_in = static_cast<const char *>(ep->d_in.p);
    for (int q = 0; q < 6; ++q) std::memcpy(h_in + (size_t)q * P * sizeof(double), planes[q], P * sizeof(double));
    if (theta0) std::memcpy(h_in + th0_off, theta0, Kz * sizeof(double));
    if (len) std::memcpy(h_in + len_off, len, Kz * sizeof(int32_t));
    RP_TRY(ep, hipMemcpyAsync(ep->d_in.p, ep->h_in.p, in_bytes, hipMemcpyHostToDevice, ep->stream));
    char *dv = static_cast<char *>(ep->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(dv);
    double *d_block = reinterpret_cast<double *>(dv + blk_off), *d_cost = reinterpret_cast<double *>(dv + cost_off);
    double *d_risk = reinterpret_cast<double *>(dv + risk_off);
    uint32_t *d_status = reinterpret_cast<uint32_t *>(dv + st_off);
    int32_t *d_hit = reinterpret_cast<int32_t *>(dv + mh_off);
    int32_t *d_first_pose = reinterpret_cast<int32_t *>(dv + fp_off), *d_first_seg = reinterpret_cast<int32_t *>(dv + fs_off);
    double *d_planes = reinterpret_cast<double *>(dv + pl_off);
    const double *d_six = reinterpret_cast<const double *>(d_in);
    const int32_t *d_len = len ? reinterpret_cast<const int32_t *>(d_in + len_off) : nullptr;
    const double *d_th0 = theta0 ? reinterpret_cast<const double *>(d_in + th0_off) : nullptr;
    const LfKin kin = {p->constraint_mask, p->low_vel_mode ? 1 : 0, p->dt, p->wheelbase, p->a_max, p->v_switch, p->v_delta_max,
                       std::tan(p->delta_max) / p->wheelbase, p->x0_orientation};
    const PkCost cc = pk_cost_of(cost);
    EpPlanes all;
    for (int q = 0; q < LF_PLANES; ++q) all.plane[q] = q < 3 || outs[q] ? d_planes + (size_t)q * P : nullptr;
    const bool rows_in_lds = ep->tb.n_seg <= EP_LF_LDS_ROWS;
    const auto lift = rows_in_lds ? rp_epick_lift_kernel<true> : rp_epick_lift_kernel<false>;
    const size_t lds_bytes = rows_in_lds ? (size_t)ep->tb.n_seg * LF_ROW * sizeof(double) : 0;
    hipLaunchKernelGGL(lift, dim3((unsigned)((K + EP_WAVES - 1) / EP_WAVES)), dim3(EP_BLOCK), lds_bytes, ep->stream, ep->tb, kin, cc, d_six, d_len, d_th0,
                       (long long)K, (int)n_poses, (const unsigned long long *)nullptr, (double *)nullptr, all, d_status, d_cost);
    RP_TRY(ep, hipGetLastError());
    if (mode != 0) {
        RP_TRY(ep, hipMemsetAsync(d_first_pose, 0x7f, 2 * mat_bytes, ep->stream));
        const int nchunk = (n_poses + 63) / 64;
        const long long waves = (long long)K * nchunk;   // <= 2^24: the grid's x fits
        const dim3 grid((unsigned)((waves + EP_WAVES - 1) / EP_WAVES), (unsigned)((M + EP_MEMBER_BLOCK - 1) / EP_MEMBER_BLOCK));
        const bool shapes_in_lds = ep->stat.n_sobb + ep->stat.n_tri + ep->stat.n_circ <= EP_CK_LDS_ROWS;
        const auto collide = shapes_in_lds ? rp_epick_collide_kernel<true> : rp_epick_collide_kernel<false>;
        hipLaunchKernelGGL(collide, grid, dim3(EP_BLOCK), 0, ep->stream, ep->stat, ep->mb, d_planes, d_len, d_status, (int)K, (int)n_poses, nchunk, mode,
                           p->wb_rear_axle, 0.5 * p->length, 0.5 * p->width, (int)p->time_step0, (int)p->factor, d_first_pose, d_first_seg);
        RP_TRY(ep, hipGetLastError());
    }
    hipLaunchKernelGGL(rp_epick_risk_kernel, dim3((unsigned)((K + 63) / 64)), dim3(EP_RISK_BLOCK), 0, ep->stream, (int)K, M, mode, max_risk, ep->mb.weight,
                       d_status, d_first_pose, d_first_seg, d_hit, d_risk);
    RP_TRY(ep, hipGetLastError());
    hipLaunchKernelGGL(rp_epick_final_kernel, dim3(1), dim3(EP_FINAL_BLOCK), 0, ep->stream, (long long)K, mode, d_status, d_cost, d_hit, d_risk, d_red);
    RP_TRY(ep, hipGetLastError());
    if (best_states) {
        EpPlanes rows;
        for (int q = 0; q < LF_PLANES; ++q) rows.plane[q] = d_block + (size_t)EP_PLANE_ROW[q] * nz;
        hipLaunchKernelGGL(lift, dim3(1), dim3(EP_BLOCK), lds_bytes, ep->stream, ep->tb, kin, cc, d_six, d_len, d_th0, (long long)K, (int)n_poses,
                           (const unsigned long long *)d_red, d_block, rows, (uint32_t *)nullptr, (double *)nullptr);
        RP_TRY(ep, hipGetLastError());
    }
    char *h_out = static_cast<char *>(ep->h_out.p);
    RP_TRY(ep, hipMemcpyAsync(h_out, dv, front_bytes, hipMemcpyDeviceToHost, ep->stream));
    if (first_pose_hit) RP_TRY(ep, hipMemcpyAsync(h_out + h_fp_off, d_first_pose, mat_bytes, hipMemcpyDeviceToHost, ep->stream));
    if (first_segment_hit) RP_TRY(ep, hipMemcpyAsync(h_out + h_fs_off, d_first_seg, mat_bytes, hipMemcpyDeviceToHost, ep->stream));
    if (pl_bytes)
        RP_TRY(ep, hipMemcpyAsync(h_out + h_pl_off, dv + pl_off + (size_t)pl_first * P * sizeof(double), pl_bytes, hipMemcpyDeviceToHost, ep->stream));
    RP_TRY(ep, hipStreamSynchronize(ep->stream));
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    if (result) {
        const bool any = h_red[RED_BEST] < (unsigned long long)K;
        result->best = any ? (int64_t)h_red[RED_BEST] : -1;
        if (any) {
            std::memcpy(&result->best_cost, &h_red[RED_COST], sizeof(double));
            std::memcpy(&result->best_risk, &h_red[RED_BEST_RISK], sizeof(double));
        } else {
            result->best_cost = std::nan("");
            result->best_risk = std::nan("");
        }
        result->best_members_hit = any ? (int64_t)h_red[RED_BEST_HIT] : -1;
        result->n_feasible = (int64_t)h_red[RED_FEASIBLE];
        result->n_collision = (int64_t)h_red[RED_COLLISION];
        result->n_collision_before_best = (int64_t)h_red[RED_BEFORE];
        for (int q = 0; q < 8; ++q) result->reason_counts[q] = (int64_t)h_red[RED_REASON0 + q];
    }
    if (best_states) std::memcpy(best_states, h_out + blk_off, block_bytes);
    if (cost_out) std::memcpy(cost_out, h_out + cost_off, Kz * sizeof(double));
    if (risk) std::memcpy(risk, h_out + risk_off, Kz * sizeof(double));
    if (status) std::memcpy(status, h_out + st_off, Kz * sizeof(uint32_t));
    if (members_hit) std::memcpy(members_hit, h_out + mh_off, Kz * sizeof(int32_t));
    if (first_pose_hit) std::memcpy(first_pose_hit, h_out + h_fp_off, mat_bytes);
    if (first_segment_hit) std::memcpy(first_segment_hit, h_out + h_fs_off, mat_bytes);
    for (int q = 0; q < LF_PLANES; ++q)
        if (outs[q]) std::memcpy(outs[q], h_out + h_pl_off + (size_t)(q - pl_first) * P * sizeof(double), P * sizeof(double));
    return RP_OK;
}

}  // extern "C"
