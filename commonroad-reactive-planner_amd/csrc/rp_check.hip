// rp_check.hip -- librp_check.so: the batch collision checker of include/rp_check.h (MI355X / gfx950).
//
// K given trajectories x n poses x M obstacles: no sampling grid, no costs, no reference path, and nothing shared with a
// planning context.  The narrow phase is the planner's (rp_device.h: Obb, obb_obb, obb_tri, obb_circ, merge_swept), so a verdict
// is the boolean the planner's kernels produce; the tables are laid out for THIS kernel's wavefronts -- 64 consecutive poses of
// one trajectory -- not for the planner's (neighbouring candidates: clusters, slots and the static grid of rp_host.hip stay there).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_check_rules.h"   // the tables as the kernels see them, cc.collide and both tests of a chunk: shared with rp_pick.hip
#include "rp_session.h"       // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_check.h"

namespace {

constexpr int CK_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int CK_WAVES = CK_BLOCK / 64;
constexpr int CK_LDS_ROWS = 128;                // static rows staged in LDS (10 KiB per workgroup); more: read from device memory

// A lane is a pose (and the segment that starts at it), a wavefront 64 consecutive poses of one trajectory: wavefront w of the
// grid = chunk w % nchunk of trajectory w / nchunk.  poses: planes x | y | theta, each [K][n].  first_pose / first_seg hold CK_NONE
// on entry (a fill in front of the launch) and receive the smallest colliding index by one atomicMin per wavefront that has a hit.
template <bool LDS>
__global__ __launch_bounds__(CK_BLOCK) void rp_check_batch_kernel(CkTables tb, const double *poses, const int32_t *len, int K, int n, int nchunk,
                                                                  uint32_t mode, double wb_rear_axle, double hl, double hw, int t0, int factor,
                                                                  int32_t *first_pose, int32_t *first_seg, uint8_t *pose_hit,
                                                                  unsigned long long *red) {
    __shared__ double sh_rows[LDS ? CK_LDS_ROWS * CK_ROW : 1];
    if (LDS) {
        const int nd = (tb.n_sobb + tb.n_tri + tb.n_circ) * CK_ROW;   // <= CK_LDS_ROWS * CK_ROW: the host picks this variant
        for (int q = threadIdx.x; q < nd; q += CK_BLOCK) sh_rows[q] = tb.stat[q];
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { red[0] = ~0ull; red[1] = 0ull; }   // for rp_check_reduce_kernel, behind this launch
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * CK_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= (long long)K * nchunk) return;   // (a whole wavefront, behind the only barrier)
    const int k = (int)(w / nchunk), chunk = (int)(w % nchunk);
    const int i = chunk * 64 + lane;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    const bool have = i < L;
    const size_t plane = (size_t)K * (size_t)n;
    const size_t at = (size_t)k * (size_t)n + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never asked
    const Obb ego = ck_ego(poses, plane, at, wb_rear_axle, hl, hw);

    if (mode & RP_TRAJ_POSES) {
        const bool hit = ck_pose_hit<LDS>(tb, sh_rows, ego, hl, hw, t0, factor, i, have);
        if (pose_hit && i < n) pose_hit[(size_t)k * (size_t)n + (size_t)i] = hit ? 1 : 0;
        const unsigned long long b = __ballot(hit);
        if (b != 0 && lane == 0) atomicMin(&first_pose[k], chunk * 64 + (__ffsll(b) - 1));
    }
    if (mode & RP_TRAJ_SWEPT) {
        const bool hit = ck_segment_hit<LDS>(tb, sh_rows, ego, poses, plane, at, wb_rear_axle, hl, hw, t0, i, L, lane);
        const unsigned long long b = __ballot(hit);
        if (b != 0 && lane == 0) atomicMin(&first_seg[k], chunk * 64 + (__ffsll(b) - 1));
    }
}

// One lane per trajectory: CK_NONE -> -1 in the first-hit arrays, then red[0] = smallest k without a requested hit (~0: none),
// red[1] = trajectories with one -- a ballot per wavefront, one atomic each per wavefront.
__global__ __launch_bounds__(CK_BLOCK) void rp_check_reduce_kernel(int K, int32_t *first_pose, int32_t *first_seg, unsigned long long *red) {
    const int k = blockIdx.x * CK_BLOCK + threadIdx.x;
    const bool in = k < K;
    int32_t fp = in ? first_pose[k] : -1, fs = in ? first_seg[k] : -1;
    fp = fp >= CK_NONE ? -1 : fp;
    fs = fs >= CK_NONE ? -1 : fs;
    if (in) { first_pose[k] = fp; first_seg[k] = fs; }
    const bool hit = fp >= 0 || fs >= 0;
    const unsigned long long bh = __ballot(in && hit), bf = __ballot(in && !hit);
    if ((threadIdx.x & 63) == 0) {
        if (bh != 0) atomicAdd(&red[1], (unsigned long long)__popcll(bh));
        if (bf != 0) atomicMin(&red[0], (unsigned long long)(k + (__ffsll(bf) - 1)));
    }
}

}  // namespace

struct rp_checker : RpSession {
    CkTables tb = {nullptr, nullptr, 0, 0, 0, 0, 0, 0};
    RpTable d_stat, d_dyn;
};

extern "C" {

int rp_checker_abi_version(void) { return RP_CHECKER_ABI_VERSION; }

int rp_checker_create(rp_checker **out, int device) { return session_create(out, device); }

void rp_checker_destroy(rp_checker *ck) { session_destroy(ck); }

const char *rp_checker_last_error(const rp_checker *ck) { return session_last_error(ck, "null checker"); }

int rp_checker_set_obstacles(rp_checker *ck, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ,
                             const double *circ, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn) {
    if (!ck) return RP_EINVAL;
    if (!ck->stream) return fail(ck, RP_ESTATE, "rp_checker_set_obstacles: the checker has no device (rp_checker_create failed)");
    std::vector<double> a, e;
    std::string msg;
    int rc = ot_build("rp_checker_set_obstacles", n_sobb, sobb, n_tri, tri, n_circ, circ, n_dyn, n_steps, dyn, a, e, msg);
    if (rc != RP_OK) return fail(ck, rc, msg);
    if ((rc = replace_tables(ck, {{&ck->d_stat, &a}, {&ck->d_dyn, &e}})) != RP_OK) return rc;
    const bool any_dyn = !e.empty();
    ck->tb = {ck->d_stat.p, ck->d_dyn.p, n_sobb, n_tri, n_circ, any_dyn ? n_dyn : 0, any_dyn ? n_steps : 0, dyn_t0};
    return RP_OK;
}

int rp_checker_check(rp_checker *ck, const rp_params *p, uint32_t mode, int64_t K, int32_t n_poses, const double *x, const double *y,
                     const double *theta, const int32_t *len, int32_t *first_pose_hit, int32_t *first_segment_hit, uint8_t *pose_hit,
                     int64_t *first_free, int64_t *n_hit) {
    if (!ck) return RP_EINVAL;
    if (!p) return fail(ck, RP_EINVAL, "rp_checker_check: null params");
    if (p->struct_size != sizeof(rp_params)) return fail(ck, RP_EABI, "rp_checker_check: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (mode == 0 || (mode & ~(RP_TRAJ_POSES | RP_TRAJ_SWEPT)) != 0) return fail(ck, RP_EINVAL, "rp_checker_check: mode must be RP_TRAJ_POSES, RP_TRAJ_SWEPT or both");
    if (K < 0 || n_poses < 1) return fail(ck, RP_EINVAL, "rp_checker_check: K < 0 or n_poses < 1");
    if (K > RP_CHECKER_MAX_POSES || K * (int64_t)n_poses > RP_CHECKER_MAX_POSES)
        return fail(ck, RP_EINVAL, "rp_checker_check: K * n_poses beyond RP_CHECKER_MAX_POSES");
    if (!(mode & RP_TRAJ_POSES) && (first_pose_hit || pose_hit)) return fail(ck, RP_EINVAL, "rp_checker_check: first_pose_hit / pose_hit without RP_TRAJ_POSES");
    if (!(mode & RP_TRAJ_SWEPT) && first_segment_hit) return fail(ck, RP_EINVAL, "rp_checker_check: first_segment_hit without RP_TRAJ_SWEPT");
    if (K > 0 && (!x || !y || !theta)) return fail(ck, RP_EINVAL, "rp_checker_check: null poses");
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(ck, RP_EINVAL, "rp_checker_check: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (K == 0) {
        if (first_free) *first_free = -1;
        if (n_hit) *n_hit = 0;
        return RP_OK;
    }
    if (!ck->stream) return fail(ck, RP_ESTATE, "rp_checker_check: the checker has no device (rp_checker_create failed)");
    RP_TRY(ck, hipSetDevice(ck->device));
    const size_t P = (size_t)K * (size_t)n_poses;
    const size_t in_bytes = 3 * P * sizeof(double) + (len ? (size_t)K * sizeof(int32_t) : 0);
    const size_t first_off = 2 * sizeof(unsigned long long), hits_off = first_off + 2 * (size_t)K * sizeof(int32_t);
    const size_t out_bytes = hits_off + (pose_hit ? P : 0);
    const int rc = grow_call(ck, "rp_checker_check", in_bytes, out_bytes, out_bytes);
    if (rc != RP_OK) return rc;
    double *h_poses = static_cast<double *>(ck->h_in.p);
    std::memcpy(h_poses, x, P * sizeof(double));
    std::memcpy(h_poses + P, y, P * sizeof(double));
    std::memcpy(h_poses + 2 * P, theta, P * sizeof(double));
    if (len) std::memcpy(h_poses + 3 * P, len, (size_t)K * sizeof(int32_t));
    RP_TRY(ck, hipMemcpyAsync(ck->d_in.p, ck->h_in.p, in_bytes, hipMemcpyHostToDevice, ck->stream));
    char *d_out = static_cast<char *>(ck->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(d_out);
    int32_t *d_first_pose = reinterpret_cast<int32_t *>(d_out + first_off), *d_first_seg = d_first_pose + K;
    uint8_t *d_hits = pose_hit ? reinterpret_cast<uint8_t *>(d_out + hits_off) : nullptr;
    RP_TRY(ck, hipMemsetAsync(d_first_pose, 0x7f, 2 * (size_t)K * sizeof(int32_t), ck->stream));
    const double *d_poses = static_cast<const double *>(ck->d_in.p);
    const int32_t *d_len = len ? reinterpret_cast<const int32_t *>(d_poses + 3 * P) : nullptr;
    const int nchunk = (n_poses + 63) / 64;
    const long long waves = (long long)K * nchunk;
    const unsigned grid = (unsigned)((waves + CK_WAVES - 1) / CK_WAVES);
    const bool in_lds = ck->tb.n_sobb + ck->tb.n_tri + ck->tb.n_circ <= CK_LDS_ROWS;
    const auto kernel = in_lds ? rp_check_batch_kernel<true> : rp_check_batch_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(CK_BLOCK), 0, ck->stream, ck->tb, d_poses, d_len, (int)K, (int)n_poses, nchunk, mode,
                       p->wb_rear_axle, 0.5 * p->length, 0.5 * p->width, (int)p->time_step0, (int)p->factor, d_first_pose, d_first_seg, d_hits,
                       d_red);
    RP_TRY(ck, hipGetLastError());
    hipLaunchKernelGGL(rp_check_reduce_kernel, dim3((unsigned)((K + CK_BLOCK - 1) / CK_BLOCK)), dim3(CK_BLOCK), 0, ck->stream, (int)K, d_first_pose,
                       d_first_seg, d_red);
    RP_TRY(ck, hipGetLastError());
    RP_TRY(ck, hipMemcpyAsync(ck->h_out.p, ck->d_out.p, out_bytes, hipMemcpyDeviceToHost, ck->stream));
    RP_TRY(ck, hipStreamSynchronize(ck->stream));
    const char *h_out = static_cast<const char *>(ck->h_out.p);
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    if (first_free) *first_free = h_red[0] < (unsigned long long)K ? (int64_t)h_red[0] : -1;
    if (n_hit) *n_hit = (int64_t)h_red[1];
    if (first_pose_hit) std::memcpy(first_pose_hit, h_out + first_off, (size_t)K * sizeof(int32_t));
    if (first_segment_hit) std::memcpy(first_segment_hit, h_out + first_off + (size_t)K * sizeof(int32_t), (size_t)K * sizeof(int32_t));
    if (pose_hit) std::memcpy(pose_hit, h_out + hits_off, P);
    return RP_OK;
}

}  // extern "C"
