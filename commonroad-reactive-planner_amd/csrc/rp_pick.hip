// rp_pick.hip -- librp_pick.so: the pick of include/rp_pick.h (MI355X / gfx950).
//
// K given curvilinear trajectories x n poses along ONE reference path, against one set of obstacle tables: the lift of rp_lift.h, the
// default cost of rp_score.h, the collision tests of rp_check.h and ReactivePlanner._get_optimal_trajectory's choice among them, with
// the poses staying on the device between the stages.  The mapping is the family's: a lane is a pose, a wavefront 64 consecutive
// poses of one trajectory, a workgroup four wavefronts.  The per-pose lift step and the obstacle walk are the two siblings', from
// the files they are stated in once (rp_lift_rules.h with rp_lift_walk.inc, rp_check_rules.h), and the cost is stated in
// rp_pick_cost.h, for rp_epick.hip too.  What is written here is the skip of infeasible trajectories, the final stage and the host side.
//
//   rp_pick_lift_kernel      one wavefront walks one trajectory: eight planes (x, y, theta always, the rest where asked for), the
//                            kinematic verdict and the cost
//   rp_pick_collide_kernel   (trajectory, chunk) wavefronts over the kept poses; a trajectory that is not feasible returns at once
//   rp_pick_final_kernel     one workgroup: collision labels, the winner, the counts
//   rp_pick_lift_kernel      once more, one wavefront on the winner alone: its state block
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_check_rules.h"   // the obstacle tables and their builder, cc.collide and both tests of a chunk: shared with rp_check.hip
#include "rp_lift_rules.h"    // the segment row, the segment search, the step's checks: shared with rp_lift.hip
#include "rp_pick_cost.h"     // the cost's scalars and the terms of a pose: shared with rp_epick.hip
#include "rp_session.h"       // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_pick.h"

namespace {

constexpr int PK_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int PK_WAVES = PK_BLOCK / 64;
constexpr int PK_LF_LDS_ROWS = 384;             // most segment rows staged in LDS: the lift's capacity (LF_LDS_ROWS of rp_lift.hip)
constexpr int PK_CK_LDS_ROWS = 128;             // most static rows staged in LDS: the checker's capacity (CK_LDS_ROWS of rp_check.hip)
constexpr int PK_FINAL_BLOCK = 1024;            // the one workgroup of rp_pick_final_kernel
constexpr unsigned long long PK_NO_K = ~0ull;

// the scalars of a call on the device, 16 words
enum { RED_BEST, RED_COST, RED_FEASIBLE, RED_COLLISION, RED_BEFORE, RED_REASON0 /* .. + 7 */, RED_WORDS = 16 };

// the row of a state block each of the eight planes and each of the six input planes is
constexpr int PK_PLANE_ROW[LF_PLANES] = {RP_X, RP_Y, RP_THETA, RP_V, RP_A, RP_KAPPA, RP_KAPPA_DOT, RP_THETA_CL};
constexpr int PK_INPUT_ROW[6] = {RP_S, RP_S_DOT, RP_S_DDOT, RP_D, RP_D_DOT, RP_D_DDOT};

// where a launch writes each of the eight planes (nullptr: nowhere)
struct PkPlanes {
    double *plane[LF_PLANES];
};

// Wavefront w of the grid = trajectory w; it walks the trajectory as rp_lift_pose_kernel does (rp_lift_walk.inc: the same text), writes the planes the
// launch has a place for at [k][i], and adds the cost's terms of its lane's poses in ascending order -- the 64 partial sums meet in
// a fixed butterfly.  in: the six input planes, each [K][n].
// With `sel` the launch is one workgroup whose first wavefront lifts trajectory sel[0] alone into a state block (`block`,
// [RP_N_ARRAYS][n]; the planes point at its rows): the same code on the same inputs, so the rows are bit-equal to the planes of the
// launch over all K.  sel[0] beyond K: no winner, the block is NaN.
template <bool LDS>
__global__ __launch_bounds__(PK_BLOCK) void rp_pick_lift_kernel(LfTable tb, LfKin kin, PkCost cc, const double *in, const int32_t *len, const double *theta0,
                                                                long long K, int n, const unsigned long long *sel, double *block, PkPlanes out,
                                                                uint32_t *status, double *cost) {
    extern __shared__ double sh_rows[];     // n_seg rows (the launch sizes it); none if !LDS
    if (LDS) {
        const int nd = tb.n_seg * LF_ROW;   // <= PK_LF_LDS_ROWS * LF_ROW: the host picks this variant and allocates nd doubles
        for (int q = threadIdx.x; q < nd; q += PK_BLOCK) sh_rows[q] = tb.rows[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    long long k = (long long)blockIdx.x * PK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
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
            for (int q = 0; q < 6; ++q) block[(size_t)PK_INPUT_ROW[q] * (size_t)n + i] = i < L ? in[(size_t)q * P + base + i] : nan;
    }
}

// rp_check_batch_kernel over the kept poses: wavefront w of the grid = chunk w % nchunk of trajectory w / nchunk, and a trajectory
// whose verdict is not RP_LABEL_FEASIBLE returns at once.  poses: planes x | y | theta, each [K][n].  first_pose / first_seg hold
// CK_NONE on entry (a fill in front of the launch) and receive the smallest colliding index by one atomicMin per wavefront that has
// a hit.
template <bool LDS>
__global__ __launch_bounds__(PK_BLOCK) void rp_pick_collide_kernel(CkTables tb, const double *poses, const int32_t *len, const uint32_t *status, int K, int n,
                                                                   int nchunk, uint32_t mode, double wb_rear_axle, double hl, double hw, int t0, int factor,
                                                                   int32_t *first_pose, int32_t *first_seg) {
    __shared__ double sh_rows[LDS ? PK_CK_LDS_ROWS * CK_ROW : 1];
    if (LDS) {
        const int nd = (tb.n_sobb + tb.n_tri + tb.n_circ) * CK_ROW;   // <= PK_CK_LDS_ROWS * CK_ROW: the host picks this variant
        for (int q = threadIdx.x; q < nd; q += PK_BLOCK) sh_rows[q] = tb.stat[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * PK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= (long long)K * nchunk) return;   // (a whole wavefront, behind the only barrier)
    const int k = (int)(w / nchunk), chunk = (int)(w % nchunk);
    if (status[k] != RP_LABEL_FEASIBLE) return;   // wave-uniform: not kinematically feasible, not tested
    const int i = chunk * 64 + lane;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    const bool have = i < L;
    const size_t plane = (size_t)K * (size_t)n;
    const size_t at = (size_t)k * (size_t)n + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never asked
    const Obb ego = ck_ego(poses, plane, at, wb_rear_axle, hl, hw);
    if (mode & RP_TRAJ_POSES) {
        const bool hit = ck_pose_hit<LDS>(tb, sh_rows, ego, hl, hw, t0, factor, i, have);
        const unsigned long long b = __ballot(hit);
        if (b != 0 && lane == 0) atomicMin(&first_pose[k], chunk * 64 + (__ffsll(b) - 1));
    }
    if (mode & RP_TRAJ_SWEPT) {
        const bool hit = ck_segment_hit<LDS>(tb, sh_rows, ego, poses, plane, at, wb_rear_axle, hl, hw, t0, i, L, lane);
        const unsigned long long b = __ballot(hit);
        if (b != 0 && lane == 0) atomicMin(&first_seg[k], chunk * 64 + (__ffsll(b) - 1));
    }
}

// The scalars of a call, by ONE workgroup that strides over the K trajectories (no atomics, nothing to initialise, the same result
// whatever K).  First pass: CK_NONE -> -1 in the first-hit arrays of the requested tests, the collision label into status, the
// lexicographic minimum of (cost, k) over the trajectories left feasible and the counts.  Second pass: the colliding trajectories
// with (cost, k) below the winner's -- all of them when there is none.  A thread reads in the second pass what it wrote itself in the
// first.
__global__ __launch_bounds__(PK_FINAL_BLOCK) void rp_pick_final_kernel(long long K, uint32_t mode, uint32_t *status, const double *cost, int32_t *first_pose,
                                                                       int32_t *first_seg, unsigned long long *red) {
    constexpr int NW = PK_FINAL_BLOCK / 64;
    __shared__ unsigned long long sh_k[NW];
    __shared__ double sh_c[NW];
    __shared__ uint32_t sh_cnt[NW][9];   // (K <= RP_PICK_MAX_POSES = 2^24: a count fits)
    __shared__ uint32_t sh_before[NW];
    unsigned long long bestk = PK_NO_K;
    double bestc = 0.0;
    uint32_t cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // cnt[0]: kinematically feasible, cnt[8]: of them colliding
#pragma unroll 1
    for (long long k = threadIdx.x; k < K; k += PK_FINAL_BLOCK) {   // ascending: a thread keeps the first of equal costs
        const uint32_t st = status[k];
        int32_t fp = -1, fs = -1;
        if (mode & RP_TRAJ_POSES) { fp = first_pose[k]; fp = fp >= CK_NONE ? -1 : fp; first_pose[k] = fp; }
        if (mode & RP_TRAJ_SWEPT) { fs = first_seg[k]; fs = fs >= CK_NONE ? -1 : fs; first_seg[k] = fs; }
        if (RP_STATUS_LABEL(st) == RP_LABEL_FEASIBLE) {
            ++cnt[0];
            if (fp >= 0 || fs >= 0) {
                ++cnt[8];
                uint32_t step = (uint32_t)(fp >= 0 ? fp : fs);
                step = step > 0xFFFu ? 0xFFFu : step;
                status[k] = RP_LABEL_INFEASIBLE_COLLISION | (step << 8);
            } else {
                const double cv = cost[k];
                if (cv == cv && (bestk == PK_NO_K || cv < bestc)) { bestc = cv; bestk = (unsigned long long)k; }
            }
        } else {
            const uint32_t r = RP_STATUS_REASON(st);
#pragma unroll
            for (uint32_t q = 1; q < 8; ++q) cnt[q] += r == q ? 1u : 0u;
        }
    }
    auto merge = [&](unsigned long long ok, double oc) {
        if (ok != PK_NO_K && (bestk == PK_NO_K || oc < bestc || (oc == bestc && ok < bestk))) { bestc = oc; bestk = ok; }
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
        for (long long k = threadIdx.x; k < K; k += PK_FINAL_BLOCK) {
            if (RP_STATUS_LABEL(status[k]) != RP_LABEL_INFEASIBLE_COLLISION) continue;
            const double cv = cost[k];
            before += (bestk == PK_NO_K || cv < bestc || (cv == bestc && (unsigned long long)k < bestk)) ? 1u : 0u;
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
    }
}

}  // namespace

struct rp_pick : RpSession {
    LfTable tb = {nullptr, 0, 0, 0.0, 0.0, 0.0};
    CkTables ob = {nullptr, nullptr, 0, 0, 0, 0, 0, 0};
    RpTable d_rows, d_stat, d_dyn;
};

extern "C" {

int rp_pick_abi_version(void) { return RP_PICK_ABI_VERSION; }

int rp_pick_create(rp_pick **out, int device) { return session_create(out, device); }

void rp_pick_destroy(rp_pick *pk) { session_destroy(pk); }

const char *rp_pick_last_error(const rp_pick *pk) { return session_last_error(pk, "null pick object"); }

int rp_pick_set_reference(rp_pick *pk, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta, const double *ref_curv,
                          const double *ref_curv_d, double proj_domain_d_limit) {
    if (!pk) return RP_EINVAL;
    if (!pk->stream) return fail(pk, RP_ESTATE, "rp_pick_set_reference: the object has no device (rp_pick_create failed)");
    std::vector<double> rows;
    std::string msg;
    int rc = lf_build_rows("rp_pick_set_reference", n, ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, proj_domain_d_limit, rows, msg);
    if (rc != RP_OK) return fail(pk, rc, msg);
    if ((rc = replace_tables(pk, {{&pk->d_rows, &rows}})) != RP_OK) return rc;
    pk->tb = {pk->d_rows.p, n - 1, lf_search_iters(n), ref_pos[0], ref_pos[n - 1], proj_domain_d_limit};
    return RP_OK;
}

int rp_pick_set_obstacles(rp_pick *pk, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ,
                          int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn) {
    if (!pk) return RP_EINVAL;
    if (!pk->stream) return fail(pk, RP_ESTATE, "rp_pick_set_obstacles: the object has no device (rp_pick_create failed)");
    std::vector<double> a, e;
    std::string msg;
    int rc = ot_build("rp_pick_set_obstacles", n_sobb, sobb, n_tri, tri, n_circ, circ, n_dyn, n_steps, dyn, a, e, msg);
    if (rc != RP_OK) return fail(pk, rc, msg);
    if ((rc = replace_tables(pk, {{&pk->d_stat, &a}, {&pk->d_dyn, &e}})) != RP_OK) return rc;
    const bool any_dyn = !e.empty();
    pk->ob = {pk->d_stat.p, pk->d_dyn.p, n_sobb, n_tri, n_circ, any_dyn ? n_dyn : 0, any_dyn ? n_steps : 0, dyn_t0};
    return RP_OK;
}

int rp_pick_select(rp_pick *pk, const rp_params *p, const rp_cost *cost, uint32_t mode, int64_t K, int32_t n_poses, const double *s, const double *s_dot,
                   const double *s_ddot, const double *d, const double *d_dot, const double *d_ddot, const int32_t *len, const double *theta0,
                   uint32_t flags, double *x, double *y, double *theta, double *v, double *a, double *kappa, double *kappa_dot, double *theta_cl,
                   uint32_t *status, double *cost_out, int32_t *first_pose_hit, int32_t *first_segment_hit, rp_pick_result *result, double *best_states) {
    if (!pk) return RP_EINVAL;
    if (!p || !cost) return fail(pk, RP_EINVAL, "rp_pick_select: null params or cost");
    if (p->struct_size != sizeof(rp_params)) return fail(pk, RP_EABI, "rp_pick_select: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (cost->struct_size != sizeof(rp_cost)) return fail(pk, RP_EABI, "rp_pick_select: rp_cost.struct_size is not this library's sizeof(rp_cost)");
    if (result && result->struct_size != sizeof(rp_pick_result))
        return fail(pk, RP_EABI, "rp_pick_select: rp_pick_result.struct_size is not this library's sizeof(rp_pick_result)");
    if ((mode & ~(RP_TRAJ_POSES | RP_TRAJ_SWEPT)) != 0) return fail(pk, RP_EINVAL, "rp_pick_select: mode has a bit besides RP_TRAJ_POSES and RP_TRAJ_SWEPT");
    if (K < 0 || n_poses < 1) return fail(pk, RP_EINVAL, "rp_pick_select: K < 0 or n_poses < 1");
    if (K > RP_PICK_MAX_POSES || K * (int64_t)n_poses > RP_PICK_MAX_POSES) return fail(pk, RP_EINVAL, "rp_pick_select: K * n_poses beyond RP_PICK_MAX_POSES");
    if (flags != 0) return fail(pk, RP_EINVAL, "rp_pick_select: unknown flags");
    if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fail(pk, RP_EINVAL, "rp_pick_select: dt must be positive");
    if (cost->kind != RP_COST_DEFAULT && cost->kind != RP_COST_FAILSAFE)
        return fail(pk, RP_EINVAL, "rp_pick_select: cost kind must be RP_COST_DEFAULT or RP_COST_FAILSAFE");
    const double desired[3] = {cost->desired_speed, cost->desired_d, cost->desired_s};
    for (double q : desired)
        if (!std::isnan(q) && !std::isfinite(q)) return fail(pk, RP_EINVAL, "rp_pick_select: a desired value of the cost is infinite");
    if (!(mode & RP_TRAJ_POSES) && first_pose_hit) return fail(pk, RP_EINVAL, "rp_pick_select: first_pose_hit without RP_TRAJ_POSES");
    if (!(mode & RP_TRAJ_SWEPT) && first_segment_hit) return fail(pk, RP_EINVAL, "rp_pick_select: first_segment_hit without RP_TRAJ_SWEPT");
    const double *planes[6] = {s, s_dot, s_ddot, d, d_dot, d_ddot};
    if (K > 0)
        for (const double *q : planes)
            if (!q) return fail(pk, RP_EINVAL, "rp_pick_select: a null input plane");
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(pk, RP_EINVAL, "rp_pick_select: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (!pk->stream) return fail(pk, RP_ESTATE, "rp_pick_select: the object has no device (rp_pick_create failed)");
    if (!pk->tb.rows) return fail(pk, RP_ESTATE, "rp_pick_select: no reference set (rp_pick_set_reference)");
    const size_t nz = (size_t)n_poses, block_bytes = (size_t)RP_N_ARRAYS * nz * sizeof(double);
    if (K == 0) {
        if (result) {
            result->best = -1; result->best_cost = std::nan("");
            result->n_feasible = 0; result->n_collision = 0; result->n_collision_before_best = 0;
            std::memset(result->reason_counts, 0, sizeof(result->reason_counts));
        }
        if (best_states)
            for (size_t q = 0; q < (size_t)RP_N_ARRAYS * nz; ++q) best_states[q] = std::nan("");
        return RP_OK;
    }
    RP_TRY(pk, hipSetDevice(pk->device));
    const size_t P = (size_t)K * nz, Kz = (size_t)K;
    // inputs: the six planes | theta0? [K] | len? [K]
    const size_t th0_off = 6 * P * sizeof(double), len_off = th0_off + (theta0 ? Kz * sizeof(double) : 0);
    const size_t in_bytes = len_off + (len ? Kz * sizeof(int32_t) : 0);
    // results on the device: scalars | the winner's block [RP_N_ARRAYS][n] | cost [K] | status [K] | first_pose [K] | first_seg [K] |
    // (8-byte aligned) the eight planes in the order of the arguments.  A call copies back the front of it as far as it asks for,
    // and of the planes the run from the first to the last one it asks for; planes behind the last one that is written have no room.
    const size_t blk_off = RED_WORDS * sizeof(unsigned long long), cost_off = blk_off + block_bytes, st_off = cost_off + Kz * sizeof(double);
    const size_t fp_off = st_off + Kz * sizeof(uint32_t), fs_off = fp_off + Kz * sizeof(int32_t), pl_off = align8(fs_off + Kz * sizeof(int32_t));
    double *const outs[LF_PLANES] = {x, y, theta, v, a, kappa, kappa_dot, theta_cl};
    int pl_first = LF_PLANES, pl_end = 0;
    for (int q = 0; q < LF_PLANES; ++q)
        if (outs[q]) { pl_first = q < pl_first ? q : pl_first; pl_end = q + 1; }
    const int n_dev_planes = pl_end > 3 ? pl_end : 3;   // x, y, theta are kept for the collision test whoever asks
    const size_t dev_bytes = pl_off + (size_t)n_dev_planes * P * sizeof(double);
    const size_t front_bytes = first_segment_hit ? pl_off : first_pose_hit ? fs_off : status ? fp_off : cost_out ? st_off : best_states ? cost_off : blk_off;
    const size_t pl_bytes = pl_end > pl_first ? (size_t)(pl_end - pl_first) * P * sizeof(double) : 0;
    const size_t h_pl_off = align8(front_bytes);
    const int rc = grow_call(pk, "rp_pick", in_bytes, h_pl_off + pl_bytes, dev_bytes);
    if (rc != RP_OK) return rc;
    char *h_in = static_cast<char *>(pk->h_in.p);
    const char *d_in = static_cast<const char *>(pk->d_in.p);
    for (int q = 0; q < 6; ++q) std::memcpy(h_in + (size_t)q * P * sizeof(double), planes[q], P * sizeof(double));
    if (theta0) std::memcpy(h_in + th0_off, theta0, Kz * sizeof(double));
    if (len) std::memcpy(h_in + len_off, len, Kz * sizeof(int32_t));
    RP_TRY(pk, hipMemcpyAsync(pk->d_in.p, pk->h_in.p, in_bytes, hipMemcpyHostToDevice, pk->stream));
    char *dv = static_cast<char *>(pk->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(dv);
    double *d_block = reinterpret_cast<double *>(dv + blk_off), *d_cost = reinterpret_cast<double *>(dv + cost_off);
    uint32_t *d_status = reinterpret_cast<uint32_t *>(dv + st_off);
    int32_t *d_first_pose = reinterpret_cast<int32_t *>(dv + fp_off), *d_first_seg = reinterpret_cast<int32_t *>(dv + fs_off);
    double *d_planes = reinterpret_cast<double *>(dv + pl_off);
    const double *d_six = reinterpret_cast<const double *>(d_in);
    const int32_t *d_len = len ? reinterpret_cast<const int32_t *>(d_in + len_off) : nullptr;
    const double *d_th0 = theta0 ? reinterpret_cast<const double *>(d_in + th0_off) : nullptr;
    const LfKin kin = {p->constraint_mask, p->low_vel_mode ? 1 : 0, p->dt, p->wheelbase, p->a_max, p->v_switch, p->v_delta_max,
                       std::tan(p->delta_max) / p->wheelbase, p->x0_orientation};
    const PkCost cc = pk_cost_of(cost);
    PkPlanes all;
    for (int q = 0; q < LF_PLANES; ++q) all.plane[q] = q < 3 || outs[q] ? d_planes + (size_t)q * P : nullptr;
    const bool rows_in_lds = pk->tb.n_seg <= PK_LF_LDS_ROWS;
    const auto lift = rows_in_lds ? rp_pick_lift_kernel<true> : rp_pick_lift_kernel<false>;
    const size_t lds_bytes = rows_in_lds ? (size_t)pk->tb.n_seg * LF_ROW * sizeof(double) : 0;
    hipLaunchKernelGGL(lift, dim3((unsigned)((K + PK_WAVES - 1) / PK_WAVES)), dim3(PK_BLOCK), lds_bytes, pk->stream, pk->tb, kin, cc, d_six, d_len, d_th0,
                       (long long)K, (int)n_poses, (const unsigned long long *)nullptr, (double *)nullptr, all, d_status, d_cost);
    RP_TRY(pk, hipGetLastError());
    if (mode != 0) {
        RP_TRY(pk, hipMemsetAsync(d_first_pose, 0x7f, 2 * Kz * sizeof(int32_t), pk->stream));
        const int nchunk = (n_poses + 63) / 64;
        const long long waves = (long long)K * nchunk;
        const bool shapes_in_lds = pk->ob.n_sobb + pk->ob.n_tri + pk->ob.n_circ <= PK_CK_LDS_ROWS;
        const auto collide = shapes_in_lds ? rp_pick_collide_kernel<true> : rp_pick_collide_kernel<false>;
        hipLaunchKernelGGL(collide, dim3((unsigned)((waves + PK_WAVES - 1) / PK_WAVES)), dim3(PK_BLOCK), 0, pk->stream, pk->ob, d_planes, d_len, d_status,
                           (int)K, (int)n_poses, nchunk, mode, p->wb_rear_axle, 0.5 * p->length, 0.5 * p->width, (int)p->time_step0, (int)p->factor,
                           d_first_pose, d_first_seg);
        RP_TRY(pk, hipGetLastError());
    }
    hipLaunchKernelGGL(rp_pick_final_kernel, dim3(1), dim3(PK_FINAL_BLOCK), 0, pk->stream, (long long)K, mode, d_status, d_cost, d_first_pose, d_first_seg, d_red);
    RP_TRY(pk, hipGetLastError());
    if (best_states) {
        PkPlanes rows;
        for (int q = 0; q < LF_PLANES; ++q) rows.plane[q] = d_block + (size_t)PK_PLANE_ROW[q] * nz;
        hipLaunchKernelGGL(lift, dim3(1), dim3(PK_BLOCK), lds_bytes, pk->stream, pk->tb, kin, cc, d_six, d_len, d_th0, (long long)K, (int)n_poses,
                           (const unsigned long long *)d_red, d_block, rows, (uint32_t *)nullptr, (double *)nullptr);
        RP_TRY(pk, hipGetLastError());
    }
    char *h_out = static_cast<char *>(pk->h_out.p);
    RP_TRY(pk, hipMemcpyAsync(h_out, dv, front_bytes, hipMemcpyDeviceToHost, pk->stream));
    if (pl_bytes)
        RP_TRY(pk, hipMemcpyAsync(h_out + h_pl_off, dv + pl_off + (size_t)pl_first * P * sizeof(double), pl_bytes, hipMemcpyDeviceToHost, pk->stream));
    RP_TRY(pk, hipStreamSynchronize(pk->stream));
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    if (result) {
        const bool any = h_red[RED_BEST] < (unsigned long long)K;
        result->best = any ? (int64_t)h_red[RED_BEST] : -1;
        if (any) std::memcpy(&result->best_cost, &h_red[RED_COST], sizeof(double));
        else result->best_cost = std::nan("");
        result->n_feasible = (int64_t)h_red[RED_FEASIBLE];
        result->n_collision = (int64_t)h_red[RED_COLLISION];
        result->n_collision_before_best = (int64_t)h_red[RED_BEFORE];
        for (int q = 0; q < 8; ++q) result->reason_counts[q] = (int64_t)h_red[RED_REASON0 + q];
    }
    if (best_states) std::memcpy(best_states, h_out + blk_off, block_bytes);
    if (cost_out) std::memcpy(cost_out, h_out + cost_off, Kz * sizeof(double));
    if (status) std::memcpy(status, h_out + st_off, Kz * sizeof(uint32_t));
    if (first_pose_hit) std::memcpy(first_pose_hit, h_out + fp_off, Kz * sizeof(int32_t));
    if (first_segment_hit) std::memcpy(first_segment_hit, h_out + fs_off, Kz * sizeof(int32_t));
    for (int q = 0; q < LF_PLANES; ++q)
        if (outs[q]) std::memcpy(outs[q], h_out + h_pl_off + (size_t)(q - pl_first) * P * sizeof(double), P * sizeof(double));
    return RP_OK;
}

}  // extern "C"
