// rp_lift.hip -- librp_lift.so: the lift of include/rp_lift.h (MI355X / gfx950).
//
// K given curvilinear trajectories x n poses along ONE reference path: per pose the Cartesian state (x, y, theta, v, a, kappa,
// kappa_dot, theta_cl as ReactivePlanner._check_kinematics computes them) and the step's five kinematic checks, per trajectory the
// verdict, per call the first feasible trajectory and the counts.  The mapping is the family's (rp_score.hip): a lane is a pose, a
// wavefront 64 consecutive poses of one trajectory, a workgroup four wavefronts.  Unlike the siblings' poses these depend on their
// predecessor (the yaw rate, the curvature rate, and the orientation a vehicle at standstill keeps), so ONE wavefront walks the
// whole trajectory, 64 poses at a time, and hands three values from one chunk to the next.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_lift_rules.h"   // the segment row, the segment search, the step's checks: shared with rp_pick.hip
#include "rp_session.h"      // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_lift.h"

namespace {

constexpr int LF_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int LF_WAVES = LF_BLOCK / 64;
constexpr int LF_LDS_ROWS = 384;                // most segment rows staged in LDS (128 B each, 48 KiB); more: read from device memory
constexpr int LF_FINAL_BLOCK = 1024;            // the one workgroup of rp_lift_final_kernel
// Wavefront w of the grid = trajectory w; in chunk c its lane holds pose 64 c + lane.  in: the six planes s, s_dot, s_ddot, d,
// d_dot, d_ddot, each [K][n]; out: the eight planes of LF_PLANES, each [K][n] (NaN from the pose that stops the trajectory and behind
// its end); status [K].
template <bool LDS>
__global__ __launch_bounds__(LF_BLOCK) void rp_lift_pose_kernel(LfTable tb, LfKin kin, const double *in, const int32_t *len, const double *theta0,
                                                                long long K, int n, double *out, uint32_t *status) {
    extern __shared__ double sh_rows[];     // n_seg rows (the launch sizes it: a short path leaves room for more workgroups per CU); none if !LDS
    if (LDS) {
        const int nd = tb.n_seg * LF_ROW;   // <= LF_LDS_ROWS * LF_ROW: the host picks this variant and allocates nd doubles
        for (int q = threadIdx.x; q < nd; q += LF_BLOCK) sh_rows[q] = tb.rows[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * LF_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (k >= K) return;   // (a whole wavefront, behind the only barrier)
    const LfRows<LDS> row = {sh_rows, tb.rows};
    const size_t P = (size_t)K * (size_t)n, base = (size_t)k * (size_t)n;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    // the walk itself is text shared with rp_pick.hip; here every pose goes to the eight planes at [k][i]
#define LF_PUT_NAN(I) \
    _Pragma("unroll") for (int q = 0; q < LF_PLANES; ++q) out[(size_t)q * P + base + (I)] = nan
#define LF_PUT_POSE(I, X, Y, TH, V, A, KP, KPD, THCL, LIVE, S, D) \
    {                                                              \
        double *o = out + base + (I);                              \
        o[0] = X;                                                  \
        o[P] = Y;                                                  \
        o[2 * P] = TH;                                             \
        o[3 * P] = V;                                              \
        o[4 * P] = A;                                              \
        o[5 * P] = KP;                                             \
        o[6 * P] = KPD;                                            \
        o[7 * P] = THCL;                                           \
    }
#include "rp_lift_walk.inc"
#undef LF_PUT_NAN
#undef LF_PUT_POSE
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t ob = __shfl_xor(best, o);
        best = ob < best ? ob : best;
    }
    if (lane == 0) {
        uint32_t st = RP_LABEL_FEASIBLE;
        if (best != LF_KEY_NONE) {
            uint32_t step = (best & ~LF_KEY_LATE) >> 3;
            step = step > 0xFFFu ? 0xFFFu : step;
            st = RP_LABEL_INFEASIBLE_KINEMATIC | ((best & 7u) << 4) | (step << 8);
        }
        status[k] = st;
    }
}

// rp_lift_points: lane = point of the flat batch
template <bool LDS>
__global__ __launch_bounds__(LF_BLOCK) void rp_lift_points_kernel(LfTable tb, const double *s_in, const double *d_in, long long n, double *x, double *y,
                                                                  int32_t *seg_out) {
    extern __shared__ double sh_rows[];
    if (LDS) {
        const int nd = tb.n_seg * LF_ROW;
        for (int q = threadIdx.x; q < nd; q += LF_BLOCK) sh_rows[q] = tb.rows[q];
        __syncthreads();
    }
    const long long i = (long long)blockIdx.x * LF_BLOCK + threadIdx.x;
    const bool have = i < n;
    const LfRows<LDS> row = {sh_rows, tb.rows};
    const double s = s_in[have ? i : 0], d = d_in[have ? i : 0];
    const int seg = find_segment(row, tb.n_seg, tb.iters, s);
    if (!have) return;
    const bool on = lf_finite(s) && lf_finite(d) && s >= tb.pos_first && s <= tb.pos_last && fabs(d) <= tb.d_limit;
    const double lam = (s - row(seg, R_POS)) / row(seg, R_DPOS);
    const double tx = row(seg, R_TX) + lam * row(seg, R_DTX), ty = row(seg, R_TY) + lam * row(seg, R_DTY), tl = sqrt(tx * tx + ty * ty);
    const double px = row(seg, R_PX) + lam * row(seg, R_EX), py = row(seg, R_PY) + lam * row(seg, R_EY);
    const double nan = __builtin_nan("");
    x[i] = on ? px - d * (ty / tl) : nan;
    y[i] = on ? py + d * (tx / tl) : nan;
    seg_out[i] = on ? seg : -1;
}

// The scalars of a call, by ONE workgroup that strides over the K verdicts (no atomics, nothing to initialise, the same result
// whatever K): red[0] = the smallest feasible k (~0: none), red[1] = feasible trajectories, red[2 + r] = trajectories with reason r
// (r = 0 .. 7; 0 counts nothing).
__global__ __launch_bounds__(LF_FINAL_BLOCK) void rp_lift_final_kernel(long long K, const uint32_t *status, unsigned long long *red) {
    constexpr int NW = LF_FINAL_BLOCK / 64;
    __shared__ unsigned long long sh_k[NW];
    __shared__ uint32_t sh_cnt[NW][8];   // (K <= RP_LIFT_MAX_POSES = 2^24: a count fits)
    unsigned long long firstk = ~0ull;
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // cnt[0]: feasible
#pragma unroll 1
    for (long long k = threadIdx.x; k < K; k += LF_FINAL_BLOCK) {   // ascending: a thread keeps its first
        const uint32_t st = status[k];
        if (RP_STATUS_LABEL(st) == RP_LABEL_FEASIBLE) {
            ++cnt[0];
            if (firstk == ~0ull) firstk = (unsigned long long)k;
        } else {
            const uint32_t r = RP_STATUS_REASON(st);
#pragma unroll
            for (uint32_t q = 1; q < 8; ++q) cnt[q] += r == q ? 1u : 0u;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long ok = __shfl_xor(firstk, off);
        firstk = ok < firstk ? ok : firstk;
#pragma unroll
        for (int q = 0; q < 8; ++q) cnt[q] += __shfl_xor(cnt[q], off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_k[wave] = firstk;
#pragma unroll
        for (int q = 0; q < 8; ++q) sh_cnt[wave][q] = cnt[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int w = 1; w < NW; ++w) {
            firstk = sh_k[w] < firstk ? sh_k[w] : firstk;
#pragma unroll
            for (int q = 0; q < 8; ++q) cnt[q] += sh_cnt[w][q];
        }
        red[0] = firstk;
        red[1] = cnt[0];
        red[2] = 0ull;
#pragma unroll
        for (int q = 1; q < 8; ++q) red[2 + q] = cnt[q];
    }
}

// rp_lift_points' one scalar, by one workgroup: the points whose segment is -1.
__global__ __launch_bounds__(LF_FINAL_BLOCK) void rp_lift_outside_kernel(long long n, const int32_t *seg, unsigned long long *red) {
    __shared__ unsigned long long sh[LF_FINAL_BLOCK / 64];
    unsigned long long cnt = 0;
    for (long long i = threadIdx.x; i < n; i += LF_FINAL_BLOCK) cnt += seg[i] < 0 ? 1ull : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < LF_FINAL_BLOCK / 64; ++w) cnt += sh[w];
        red[0] = cnt;
    }
}

}  // namespace

struct rp_lift : RpSession {
    LfTable tb = {nullptr, 0, 0, 0.0, 0.0, 0.0};
    RpTable d_rows;
};

extern "C" {

int rp_lift_abi_version(void) { return RP_LIFT_ABI_VERSION; }

int rp_lift_create(rp_lift **out, int device) { return session_create(out, device); }

void rp_lift_destroy(rp_lift *lf) { session_destroy(lf); }

const char *rp_lift_last_error(const rp_lift *lf) { return session_last_error(lf, "null lift object"); }

int rp_lift_set_reference(rp_lift *lf, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta, const double *ref_curv,
                          const double *ref_curv_d, double proj_domain_d_limit) {
    if (!lf) return RP_EINVAL;
    if (!lf->stream) return fail(lf, RP_ESTATE, "rp_lift_set_reference: the object has no device (rp_lift_create failed)");
    std::vector<double> rows;
    std::string msg;
    const int built = lf_build_rows("rp_lift_set_reference", n, ref_xy, ref_pos, ref_theta, ref_curv, ref_curv_d, proj_domain_d_limit, rows, msg);
    if (built != RP_OK) return fail(lf, built, msg);
    const int rc = replace_tables(lf, {{&lf->d_rows, &rows}});
    if (rc != RP_OK) return rc;
    lf->tb = {lf->d_rows.p, n - 1, lf_search_iters(n), ref_pos[0], ref_pos[n - 1], proj_domain_d_limit};
    return RP_OK;
}

int rp_lift_points(rp_lift *lf, int64_t n_points, const double *s, const double *d, double *x, double *y, int32_t *segment, int64_t *n_outside) {
    if (!lf) return RP_EINVAL;
    if (n_points < 0 || n_points > RP_LIFT_MAX_POSES) return fail(lf, RP_EINVAL, "rp_lift_points: n_points < 0 or beyond RP_LIFT_MAX_POSES");
    if (n_points > 0 && (!s || !d)) return fail(lf, RP_EINVAL, "rp_lift_points: null points");
    if (!lf->stream) return fail(lf, RP_ESTATE, "rp_lift_points: the object has no device (rp_lift_create failed)");
    if (!lf->tb.rows) return fail(lf, RP_ESTATE, "rp_lift_points: no reference set (rp_lift_set_reference)");
    if (n_points == 0) {
        if (n_outside) *n_outside = 0;
        return RP_OK;
    }
    RP_TRY(lf, hipSetDevice(lf->device));
    const size_t P = (size_t)n_points;
    const size_t in_bytes = 2 * P * sizeof(double);
    // results on the device: scalar | x [P] | y [P] | segment [P]
    const size_t x_off = 8 * sizeof(unsigned long long), y_off = x_off + P * sizeof(double), seg_off = y_off + P * sizeof(double);
    const size_t out_bytes = seg_off + P * sizeof(int32_t);
    const int rc = grow_call(lf, "rp_lift", in_bytes, out_bytes, out_bytes);
    if (rc != RP_OK) return rc;
    double *h_in = static_cast<double *>(lf->h_in.p);
    std::memcpy(h_in, s, P * sizeof(double));
    std::memcpy(h_in + P, d, P * sizeof(double));
    RP_TRY(lf, hipMemcpyAsync(lf->d_in.p, lf->h_in.p, in_bytes, hipMemcpyHostToDevice, lf->stream));
    const double *d_s = static_cast<const double *>(lf->d_in.p);
    char *dv = static_cast<char *>(lf->d_out.p);
    int32_t *d_seg = reinterpret_cast<int32_t *>(dv + seg_off);
    const bool in_lds = lf->tb.n_seg <= LF_LDS_ROWS;
    const auto kernel = in_lds ? rp_lift_points_kernel<true> : rp_lift_points_kernel<false>;
    const size_t lds_bytes = in_lds ? (size_t)lf->tb.n_seg * LF_ROW * sizeof(double) : 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_points + LF_BLOCK - 1) / LF_BLOCK)), dim3(LF_BLOCK), lds_bytes, lf->stream, lf->tb, d_s, d_s + P,
                       (long long)n_points, reinterpret_cast<double *>(dv + x_off), reinterpret_cast<double *>(dv + y_off), d_seg);
    RP_TRY(lf, hipGetLastError());
    hipLaunchKernelGGL(rp_lift_outside_kernel, dim3(1), dim3(LF_FINAL_BLOCK), 0, lf->stream, (long long)n_points, d_seg,
                       reinterpret_cast<unsigned long long *>(dv));
    RP_TRY(lf, hipGetLastError());
    RP_TRY(lf, hipMemcpyAsync(lf->h_out.p, lf->d_out.p, out_bytes, hipMemcpyDeviceToHost, lf->stream));
    RP_TRY(lf, hipStreamSynchronize(lf->stream));
    const char *h_out = static_cast<const char *>(lf->h_out.p);
    if (n_outside) *n_outside = (int64_t) * reinterpret_cast<const unsigned long long *>(h_out);
    if (x) std::memcpy(x, h_out + x_off, P * sizeof(double));
    if (y) std::memcpy(y, h_out + y_off, P * sizeof(double));
    if (segment) std::memcpy(segment, h_out + seg_off, P * sizeof(int32_t));
    return RP_OK;
}

int rp_lift_evaluate(rp_lift *lf, const rp_params *p, int64_t K, int32_t n_poses, const double *s, const double *s_dot, const double *s_ddot,
                     const double *d, const double *d_dot, const double *d_ddot, const int32_t *len, const double *theta0, uint32_t flags, double *x,
                     double *y, double *theta, double *v, double *a, double *kappa, double *kappa_dot, double *theta_cl, uint32_t *status,
                     int64_t *first_feasible, int64_t *n_feasible, int64_t *reason_counts) {
    if (!lf) return RP_EINVAL;
    if (!p) return fail(lf, RP_EINVAL, "rp_lift_evaluate: null params");
    if (p->struct_size != sizeof(rp_params)) return fail(lf, RP_EABI, "rp_lift_evaluate: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (K < 0 || n_poses < 1) return fail(lf, RP_EINVAL, "rp_lift_evaluate: K < 0 or n_poses < 1");
    if (K > RP_LIFT_MAX_POSES || K * (int64_t)n_poses > RP_LIFT_MAX_POSES)
        return fail(lf, RP_EINVAL, "rp_lift_evaluate: K * n_poses beyond RP_LIFT_MAX_POSES");
    if (flags != 0) return fail(lf, RP_EINVAL, "rp_lift_evaluate: unknown flags");
    if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fail(lf, RP_EINVAL, "rp_lift_evaluate: dt must be positive");
    const double *planes[6] = {s, s_dot, s_ddot, d, d_dot, d_ddot};
    if (K > 0)
        for (const double *q : planes)
            if (!q) return fail(lf, RP_EINVAL, "rp_lift_evaluate: a null input plane");
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(lf, RP_EINVAL, "rp_lift_evaluate: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (!lf->stream) return fail(lf, RP_ESTATE, "rp_lift_evaluate: the object has no device (rp_lift_create failed)");
    if (!lf->tb.rows) return fail(lf, RP_ESTATE, "rp_lift_evaluate: no reference set (rp_lift_set_reference)");
    if (K == 0) {
        if (first_feasible) *first_feasible = -1;
        if (n_feasible) *n_feasible = 0;
        if (reason_counts) std::memset(reason_counts, 0, 8 * sizeof(int64_t));
        return RP_OK;
    }
    RP_TRY(lf, hipSetDevice(lf->device));
    const size_t P = (size_t)K * (size_t)n_poses, Kz = (size_t)K;
    // inputs: the six planes | theta0? [K] | len? [K]
    const size_t th0_off = 6 * P * sizeof(double), len_off = th0_off + (theta0 ? Kz * sizeof(double) : 0);
    const size_t in_bytes = len_off + (len ? Kz * sizeof(int32_t) : 0);
    // results on the device: scalars | status [K] | (8-byte aligned) the eight planes in the order of the arguments; a call copies
    // back the front of it, as far as it asks for
    const size_t st_off = 16 * sizeof(unsigned long long), pl_off = align8(st_off + Kz * sizeof(uint32_t));
    const size_t dev_bytes = pl_off + (size_t)LF_PLANES * P * sizeof(double);
    double *const outs[LF_PLANES] = {x, y, theta, v, a, kappa, kappa_dot, theta_cl};
    int n_back = 0;
    for (int q = 0; q < LF_PLANES; ++q)
        if (outs[q]) n_back = q + 1;
    const size_t back_bytes = pl_off + (size_t)n_back * P * sizeof(double);
    const int rc = grow_call(lf, "rp_lift", in_bytes, back_bytes, dev_bytes);
    if (rc != RP_OK) return rc;
    char *h_in = static_cast<char *>(lf->h_in.p);
    const char *d_in = static_cast<const char *>(lf->d_in.p);
    for (int q = 0; q < 6; ++q) std::memcpy(h_in + (size_t)q * P * sizeof(double), planes[q], P * sizeof(double));
    if (theta0) std::memcpy(h_in + th0_off, theta0, Kz * sizeof(double));
    if (len) std::memcpy(h_in + len_off, len, Kz * sizeof(int32_t));
    RP_TRY(lf, hipMemcpyAsync(lf->d_in.p, lf->h_in.p, in_bytes, hipMemcpyHostToDevice, lf->stream));
    char *dv = static_cast<char *>(lf->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(dv);
    uint32_t *d_status = reinterpret_cast<uint32_t *>(dv + st_off);
    const LfKin kin = {p->constraint_mask, p->low_vel_mode ? 1 : 0, p->dt, p->wheelbase, p->a_max, p->v_switch, p->v_delta_max,
                       std::tan(p->delta_max) / p->wheelbase, p->x0_orientation};
    const bool in_lds = lf->tb.n_seg <= LF_LDS_ROWS;
    const auto kernel = in_lds ? rp_lift_pose_kernel<true> : rp_lift_pose_kernel<false>;
    const size_t lds_bytes = in_lds ? (size_t)lf->tb.n_seg * LF_ROW * sizeof(double) : 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((K + LF_WAVES - 1) / LF_WAVES)), dim3(LF_BLOCK), lds_bytes, lf->stream, lf->tb, kin,
                       reinterpret_cast<const double *>(d_in), len ? reinterpret_cast<const int32_t *>(d_in + len_off) : nullptr,
                       theta0 ? reinterpret_cast<const double *>(d_in + th0_off) : nullptr, (long long)K, (int)n_poses,
                       reinterpret_cast<double *>(dv + pl_off), d_status);
    RP_TRY(lf, hipGetLastError());
    hipLaunchKernelGGL(rp_lift_final_kernel, dim3(1), dim3(LF_FINAL_BLOCK), 0, lf->stream, (long long)K, d_status, d_red);
    RP_TRY(lf, hipGetLastError());
    RP_TRY(lf, hipMemcpyAsync(lf->h_out.p, lf->d_out.p, back_bytes, hipMemcpyDeviceToHost, lf->stream));
    RP_TRY(lf, hipStreamSynchronize(lf->stream));
    const char *h_out = static_cast<const char *>(lf->h_out.p);
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    if (first_feasible) *first_feasible = h_red[0] < (unsigned long long)K ? (int64_t)h_red[0] : -1;
    if (n_feasible) *n_feasible = (int64_t)h_red[1];
    if (reason_counts)
        for (int q = 0; q < 8; ++q) reason_counts[q] = (int64_t)h_red[2 + q];
    if (status) std::memcpy(status, h_out + st_off, Kz * sizeof(uint32_t));
    for (int q = 0; q < LF_PLANES; ++q)
        if (outs[q]) std::memcpy(outs[q], h_out + pl_off + (size_t)q * P * sizeof(double), P * sizeof(double));
    return RP_OK;
}

}  // extern "C"
