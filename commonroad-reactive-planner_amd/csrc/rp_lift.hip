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

#include "rp_device.h"
#include "rp_frontend.h"
#include "../../include/rp_lift.h"

namespace {

constexpr int LF_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int LF_WAVES = LF_BLOCK / 64;
constexpr int LF_ROW = 16;                      // doubles per segment row (below)
constexpr int LF_LDS_ROWS = 384;                // most segment rows staged in LDS (128 B each, 48 KiB); more: read from device memory
constexpr int LF_FINAL_BLOCK = 1024;            // the one workgroup of rp_lift_final_kernel
constexpr int LF_PLANES = 8;                    // x, y, theta, v, a, kappa, kappa_dot, theta_cl
constexpr uint32_t LF_KEY_NONE = 0xFFFFFFFFu;   // a trajectory's verdict key (below): nothing failed
constexpr uint32_t LF_KEY_LATE = 0x40000000u;   // ... |d| beyond the limit: behind every step's own failure

// One row per segment:
//   [0..1] p0   [2..3] e = p1 - p0   [4..5] t0   [6..7] dt = t1 - t0   [8] pos0   [9] pos1 - pos0   [10] theta0   [11] theta1 - theta0
//   [12] curv0   [13] curv1 - curv0   [14] curv_d0   [15] curv_d1 - curv_d0
enum { R_PX, R_PY, R_EX, R_EY, R_TX, R_TY, R_DTX, R_DTY, R_POS, R_DPOS, R_TH, R_DTH, R_KR, R_DKR, R_KRD, R_DKRD };

typedef const double __attribute__((address_space(3))) *lds_cdouble;

struct LfTable {
    const double *rows;
    int32_t n_seg, iters;   // iters: trips of the segment search, 2^iters >= n_seg + 1
    double pos_first, pos_last, d_limit;
};

// what the step's checks and the standstill rule read besides the pose arrays
struct LfKin {
    uint32_t mask;
    int32_t low_vel;
    double dt, wheelbase, a_max, v_switch, v_delta_max, kappa_max, theta0;
};

template <bool LDS>
struct LfRows {
    const double *lds, *dev;
    __device__ __forceinline__ double operator()(int k, int q) const {
        if constexpr (LDS) return ((lds_cdouble)lds)[k * LF_ROW + q];
        else return ((gcdouble)dev)[(size_t)k * LF_ROW + q];
    }
};

// k = the last vertex with ref_pos[k] <= s, clamped to [0, n_seg - 1]: a binary search over the rows' pos0 with a fixed trip count
// and no branch.  Whatever s is (NaN included) the result is a valid row.
template <class Row>
__device__ __forceinline__ int find_segment(const Row &row, int n_seg, int iters, double s) {
    int lo = 0, hi = n_seg;   // the number of rows with pos0 <= s lies in [lo, hi]
    for (int it = 0; it < iters; ++it) {   // wave-uniform
        const int mid = (lo + hi) >> 1;
        const bool open = lo < hi, le = row(mid < n_seg ? mid : n_seg - 1, R_POS) <= s;
        lo = open && le ? mid + 1 : lo;
        hi = open && !le ? mid : hi;
    }
    return lo > 0 ? lo - 1 : 0;
}

__device__ __forceinline__ bool lf_finite(double v) { return fabs(v) < __builtin_huge_val(); }   // (false for NaN)

// _check_constraints at one step: the first failing check in the reference's order, or RP_REASON_NONE
__device__ __forceinline__ uint32_t step_reason(const LfKin &kin, bool first, double v, double acc, double kappa, double kappa_prev, double theta,
                                                double theta_prev) {
    if ((kin.mask & RP_CHECK_VELOCITY) && v < -RP_EPS) return RP_REASON_VELOCITY;
    if ((kin.mask & RP_CHECK_KAPPA) && fabs(kappa) > kin.kappa_max) return RP_REASON_KAPPA;
    if (kin.mask & RP_CHECK_YAW_RATE) {
        const double yaw = first ? 0.0 : (theta - theta_prev) / kin.dt;
        if (fabs(rint(yaw * 1e5) / 1e5) > kin.kappa_max * v) return RP_REASON_YAW_RATE;   // round(yaw_rate, 5) of a float64
    }
    if (kin.mask & RP_CHECK_KAPPA_DOT) {
        const double wk = kin.wheelbase * kappa;                                          // 1 / cos^2(atan(wk)) = 1 + wk^2
        const double kd = first ? 0.0 : (kappa - kappa_prev) / kin.dt;
        if (fabs(kd) > kin.v_delta_max * (1.0 + wk * wk) / kin.wheelbase) return RP_REASON_KAPPA_DOT;
    }
    if (kin.mask & RP_CHECK_ACCELERATION) {
        const double hi = v > kin.v_switch ? kin.a_max * kin.v_switch / v : kin.a_max;
        if (!(-kin.a_max <= acc && acc <= hi)) return RP_REASON_ACCELERATION;
    }
    return RP_REASON_NONE;
}

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
    const double nan = __builtin_nan("");
    const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;   // the lanes up to and including this one
    // what crosses a chunk boundary: the orientation a standstill keeps, theta and kappa of the chunk's last pose, and whether the
    // trajectory was stopped
    double keep = theta0 ? theta0[k] : kin.theta0, th_last = 0.0, kp_last = 0.0;
    bool dead = false;
    uint32_t best = LF_KEY_NONE;              // the lane's smallest step << 3 | reason
    const int nchunk = (n + 63) / 64;
    for (int c = 0; c < nchunk; ++c) {        // wave-uniform
        const int i = c * 64 + lane;
        if (c * 64 >= L || dead) {            // nothing but NaN from here on
            if (i < n)
#pragma unroll
                for (int q = 0; q < LF_PLANES; ++q) out[(size_t)q * P + base + i] = nan;
            continue;
        }
        const bool have = i < L;
        const size_t at = base + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never used
        const double s = in[at], sdd = in[2 * P + at], d = in[3 * P + at], ddd = in[5 * P + at];
        double sd = in[P + at], dd = in[4 * P + at];
        if (fabs(sd) < RP_EPS) sd = 0.0;
        if (fabs(dd) < RP_EPS) dd = 0.0;
        const bool on_s = lf_finite(s) && lf_finite(sd) && lf_finite(sdd) && lf_finite(d) && lf_finite(dd) && lf_finite(ddd) && s >= tb.pos_first && s <= tb.pos_last;
        const bool off = have && !on_s;
        const uint64_t offs = __ballot(off);
        const bool before = (offs & upto & ~(1ull << lane)) != 0;   // an earlier pose of this chunk stopped the trajectory
        const int seg = find_segment(row, tb.n_seg, tb.iters, s);
        const double pos0 = row(seg, R_POS), dpos = row(seg, R_DPOS);
        const double lam = (s - pos0) / dpos;
        const double th_r = make_valid_orientation(row(seg, R_DTH) * (s - pos0) / dpos + row(seg, R_TH));   // interpolate_angle
        const double kr = row(seg, R_DKR) * lam + row(seg, R_KR), krd = row(seg, R_DKRD) * lam + row(seg, R_KRD);
        const bool moving = sd > 0.001;
        double dp, dpp;
        if (kin.low_vel) { dp = dd; dpp = ddd; }
        else {
            dp = moving ? dd / sd : 0.0;
            dpp = moving ? (ddd - dp * sdd) / (sd * sd) : 0.0;
        }
        const bool stand = !kin.low_vel && !moving;
        const double thcl_m = rp_atan(dp);
        // The standstill carry: a pose at standstill takes theta of the last pose before it that defines its own -- a scan over the
        // lanes for "the last flagged value" (the operator (a, b) -> b.flag ? b : a is associative), six shuffles; lanes without a
        // flagged pose before them in this chunk take what the chunks before left.
        double cv = thcl_m + th_r;
        int cf = stand ? 0 : 1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double tv = __shfl_up(cv, o);
            const int tf = __shfl_up(cf, o);
            if (lane >= o && !cf) { cv = tv; cf = tf; }
        }
        const double th = cf ? cv : keep;
        const double thcl = stand ? th - th_r : thcl_m;
        double sn, cs;
        rp_sincos(thcl, &sn, &cs);
        const double tn = sn / cs;
        const double q = 1.0 - kr * d, cq = cs / q;
        const double kp = (dpp + (kr * dp + krd * d) * tn) * cs * (cq * cq) + cq * kr;
        const double v = sd * (q / cs);
        const double a = sdd * q / cs + ((sd * sd) / cs) * (q * tn * (kp * q / cs - kr) - (krd * d + kr * dp));
        // the step before: the neighbour lane's, lane 0 takes the last chunk's
        double th_p = __shfl_up(th, 1), kp_p = __shfl_up(kp, 1);
        if (lane == 0) { th_p = th_last; kp_p = kp_last; }
        const bool first = i == 0;
        const uint32_t code = step_reason(kin, first, v, a, kp, kp_p, th, th_p);
        const bool in_d = fabs(d) <= tb.d_limit;
        if (have && !before) {
            const uint32_t key = off ? ((uint32_t)i << 3) | RP_REASON_OUT_OF_DOMAIN
                                 : code ? ((uint32_t)i << 3) | code
                                 : !in_d ? LF_KEY_LATE | ((uint32_t)i << 3) | RP_REASON_OUT_OF_DOMAIN : LF_KEY_NONE;
            best = key < best ? key : best;
        }
        if (i < n) {
            const bool gone = !have || before || off;
            const double tx = row(seg, R_TX) + lam * row(seg, R_DTX), ty = row(seg, R_TY) + lam * row(seg, R_DTY), tl = sqrt(tx * tx + ty * ty);
            const double px = row(seg, R_PX) + lam * row(seg, R_EX), py = row(seg, R_PY) + lam * row(seg, R_EY);
            double *o = out + base + i;
            o[0] = gone || !in_d ? nan : px - d * (ty / tl);
            o[P] = gone || !in_d ? nan : py + d * (tx / tl);
            o[2 * P] = gone ? nan : th;
            o[3 * P] = gone ? nan : v;
            o[4 * P] = gone ? nan : a;
            o[5 * P] = gone ? nan : kp;
            o[6 * P] = gone ? nan : (first ? 0.0 : kp - kp_p);
            o[7 * P] = gone ? nan : thcl;
        }
        keep = __shfl(th, 63);
        th_last = keep;
        kp_last = __shfl(kp, 63);
        dead = offs != 0;
    }
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

struct rp_lift {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    LfTable tb = {nullptr, 0, 0, 0.0, 0.0, 0.0};
    double *d_rows = nullptr;
    // inputs of a call: pinned host block and its device copy; the results on the device and a pinned host block for the part of
    // them a call asks for.  They grow on demand.
    void *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr;
    size_t cap_h_in = 0, cap_d_in = 0, cap_h_out = 0, cap_d_out = 0;
};

namespace {

int fail(rp_lift *lf, int code, const std::string &msg) {
    lf->err = msg;
    return code;
}

#define LF_TRY(lf, expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(lf, RP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

int grow(rp_lift *lf, void *&buf, size_t &cap, size_t need, bool pinned) {
    if (need <= cap) return RP_OK;
    if (buf) { LF_TRY(lf, pinned ? hipHostFree(buf) : hipFree(buf)); buf = nullptr; }
    cap = 0;
    const size_t want = need < 65536 ? 65536 : need + need / 4;
    if ((pinned ? hipHostMalloc(&buf, want, hipHostMallocDefault) : hipMalloc(&buf, want)) != hipSuccess) {
        buf = nullptr;
        return fail(lf, RP_ENOMEM, pinned ? "rp_lift: pinned host memory" : "rp_lift: device memory");
    }
    cap = want;
    return RP_OK;
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int rp_lift_abi_version(void) { return RP_LIFT_ABI_VERSION; }

int rp_lift_create(rp_lift **out, int device) {
    if (!out) return RP_EINVAL;
    *out = nullptr;
    rp_lift *lf = new (std::nothrow) rp_lift();
    if (!lf) return RP_ENOMEM;
    *out = lf;   // returned even on failure so that rp_lift_last_error works; the caller destroys it
    lf->device = device;
    int ndev = 0;
    LF_TRY(lf, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(lf, RP_EINVAL, "no such HIP device");
    LF_TRY(lf, hipSetDevice(device));
    LF_TRY(lf, hipStreamCreateWithFlags(&lf->stream, hipStreamNonBlocking));
    return RP_OK;
}

void rp_lift_destroy(rp_lift *lf) {
    if (!lf) return;
    (void)hipSetDevice(lf->device);
    if (lf->stream) (void)hipStreamSynchronize(lf->stream);
    void *dev[] = {lf->d_rows, lf->d_in, lf->d_out};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (lf->h_in) (void)hipHostFree(lf->h_in);
    if (lf->h_out) (void)hipHostFree(lf->h_out);
    if (lf->stream) (void)hipStreamDestroy(lf->stream);
    delete lf;
}

const char *rp_lift_last_error(const rp_lift *lf) { return lf ? lf->err.c_str() : "null lift object"; }

int rp_lift_set_reference(rp_lift *lf, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta, const double *ref_curv,
                          const double *ref_curv_d, double proj_domain_d_limit) {
    if (!lf) return RP_EINVAL;
    if (!lf->stream) return fail(lf, RP_ESTATE, "rp_lift_set_reference: the object has no device (rp_lift_create failed)");
    if (n < 2 || !ref_xy || !ref_pos || !ref_theta || !ref_curv || !ref_curv_d) return fail(lf, RP_EINVAL, "rp_lift_set_reference: n < 2 or a null table");
    if (!(proj_domain_d_limit > 0.0) || !std::isfinite(proj_domain_d_limit))
        return fail(lf, RP_EINVAL, "rp_lift_set_reference: proj_domain_d_limit must be positive and finite");
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(ref_xy[2 * (size_t)i]) || !std::isfinite(ref_xy[2 * (size_t)i + 1]) || !std::isfinite(ref_pos[i]) || !std::isfinite(ref_theta[i]) ||
            !std::isfinite(ref_curv[i]) || !std::isfinite(ref_curv_d[i]))
            return fail(lf, RP_EINVAL, "rp_lift_set_reference: non-finite value at vertex " + std::to_string(i));
    for (int32_t i = 0; i + 1 < n; ++i) {
        if (!(ref_pos[i + 1] > ref_pos[i])) return fail(lf, RP_EINVAL, "rp_lift_set_reference: ref_pos is not strictly increasing at vertex " + std::to_string(i + 1));
        if (ref_xy[2 * (size_t)i] == ref_xy[2 * (size_t)i + 2] && ref_xy[2 * (size_t)i + 1] == ref_xy[2 * (size_t)i + 3])
            return fail(lf, RP_EINVAL, "rp_lift_set_reference: zero-length segment " + std::to_string(i));
    }
    LF_TRY(lf, hipSetDevice(lf->device));
    LF_TRY(lf, hipStreamSynchronize(lf->stream));
    std::vector<double> rows;
    std::vector<rpfe::Pt> ref, tan;
    try {
        ref.resize(n);
        for (int32_t i = 0; i < n; ++i) ref[i] = {ref_xy[2 * (size_t)i], ref_xy[2 * (size_t)i + 1]};
        tan = rpfe::vertex_tangents(ref);
        rows.assign((size_t)(n - 1) * LF_ROW, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(lf, RP_ENOMEM, "rp_lift_set_reference: host memory");
    }
    for (int32_t k = 0; k + 1 < n; ++k) {
        double *r = rows.data() + (size_t)k * LF_ROW;
        r[R_PX] = ref[k].x; r[R_PY] = ref[k].y; r[R_EX] = ref[k + 1].x - ref[k].x; r[R_EY] = ref[k + 1].y - ref[k].y;
        r[R_TX] = tan[k].x; r[R_TY] = tan[k].y; r[R_DTX] = tan[k + 1].x - tan[k].x; r[R_DTY] = tan[k + 1].y - tan[k].y;
        r[R_POS] = ref_pos[k]; r[R_DPOS] = ref_pos[k + 1] - ref_pos[k];
        r[R_TH] = ref_theta[k]; r[R_DTH] = ref_theta[k + 1] - ref_theta[k];
        r[R_KR] = ref_curv[k]; r[R_DKR] = ref_curv[k + 1] - ref_curv[k];
        r[R_KRD] = ref_curv_d[k]; r[R_DKRD] = ref_curv_d[k + 1] - ref_curv_d[k];
        for (int q = 0; q < LF_ROW; ++q)
            if (!std::isfinite(r[q])) return fail(lf, RP_EINVAL, "rp_lift_set_reference: segment " + std::to_string(k) + " is not finite");
    }
    lf->tb = {nullptr, 0, 0, 0.0, 0.0, 0.0};   // (a failed upload leaves no table, never half of the new one)
    if (lf->d_rows) { LF_TRY(lf, hipFree(lf->d_rows)); lf->d_rows = nullptr; }
    LF_TRY(lf, hipMalloc((void **)&lf->d_rows, rows.size() * sizeof(double)));
    LF_TRY(lf, hipMemcpy(lf->d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    int32_t iters = 0;
    while (((int64_t)1 << iters) < (int64_t)n) ++iters;   // n = n_seg + 1 possible answers of the segment search
    lf->tb = {lf->d_rows, n - 1, iters, ref_pos[0], ref_pos[n - 1], proj_domain_d_limit};
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
    LF_TRY(lf, hipSetDevice(lf->device));
    const size_t P = (size_t)n_points;
    const size_t in_bytes = 2 * P * sizeof(double);
    // results on the device: scalar | x [P] | y [P] | segment [P]
    const size_t x_off = 8 * sizeof(unsigned long long), y_off = x_off + P * sizeof(double), seg_off = y_off + P * sizeof(double);
    const size_t out_bytes = seg_off + P * sizeof(int32_t);
    int rc;
    if ((rc = grow(lf, lf->h_in, lf->cap_h_in, in_bytes, true)) != RP_OK) return rc;
    if ((rc = grow(lf, lf->d_in, lf->cap_d_in, in_bytes, false)) != RP_OK) return rc;
    if ((rc = grow(lf, lf->h_out, lf->cap_h_out, out_bytes, true)) != RP_OK) return rc;
    if ((rc = grow(lf, lf->d_out, lf->cap_d_out, out_bytes, false)) != RP_OK) return rc;
    double *h_in = static_cast<double *>(lf->h_in);
    std::memcpy(h_in, s, P * sizeof(double));
    std::memcpy(h_in + P, d, P * sizeof(double));
    LF_TRY(lf, hipMemcpyAsync(lf->d_in, lf->h_in, in_bytes, hipMemcpyHostToDevice, lf->stream));
    const double *d_s = static_cast<const double *>(lf->d_in);
    char *dv = static_cast<char *>(lf->d_out);
    int32_t *d_seg = reinterpret_cast<int32_t *>(dv + seg_off);
    const bool in_lds = lf->tb.n_seg <= LF_LDS_ROWS;
    const auto kernel = in_lds ? rp_lift_points_kernel<true> : rp_lift_points_kernel<false>;
    const size_t lds_bytes = in_lds ? (size_t)lf->tb.n_seg * LF_ROW * sizeof(double) : 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n_points + LF_BLOCK - 1) / LF_BLOCK)), dim3(LF_BLOCK), lds_bytes, lf->stream, lf->tb, d_s, d_s + P,
                       (long long)n_points, reinterpret_cast<double *>(dv + x_off), reinterpret_cast<double *>(dv + y_off), d_seg);
    LF_TRY(lf, hipGetLastError());
    hipLaunchKernelGGL(rp_lift_outside_kernel, dim3(1), dim3(LF_FINAL_BLOCK), 0, lf->stream, (long long)n_points, d_seg,
                       reinterpret_cast<unsigned long long *>(dv));
    LF_TRY(lf, hipGetLastError());
    LF_TRY(lf, hipMemcpyAsync(lf->h_out, lf->d_out, out_bytes, hipMemcpyDeviceToHost, lf->stream));
    LF_TRY(lf, hipStreamSynchronize(lf->stream));
    const char *h_out = static_cast<const char *>(lf->h_out);
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
    LF_TRY(lf, hipSetDevice(lf->device));
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
    int rc;
    if ((rc = grow(lf, lf->h_in, lf->cap_h_in, in_bytes, true)) != RP_OK) return rc;
    if ((rc = grow(lf, lf->d_in, lf->cap_d_in, in_bytes, false)) != RP_OK) return rc;
    if ((rc = grow(lf, lf->h_out, lf->cap_h_out, back_bytes, true)) != RP_OK) return rc;
    if ((rc = grow(lf, lf->d_out, lf->cap_d_out, dev_bytes, false)) != RP_OK) return rc;
    char *h_in = static_cast<char *>(lf->h_in);
    const char *d_in = static_cast<const char *>(lf->d_in);
    for (int q = 0; q < 6; ++q) std::memcpy(h_in + (size_t)q * P * sizeof(double), planes[q], P * sizeof(double));
    if (theta0) std::memcpy(h_in + th0_off, theta0, Kz * sizeof(double));
    if (len) std::memcpy(h_in + len_off, len, Kz * sizeof(int32_t));
    LF_TRY(lf, hipMemcpyAsync(lf->d_in, lf->h_in, in_bytes, hipMemcpyHostToDevice, lf->stream));
    char *dv = static_cast<char *>(lf->d_out);
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
    LF_TRY(lf, hipGetLastError());
    hipLaunchKernelGGL(rp_lift_final_kernel, dim3(1), dim3(LF_FINAL_BLOCK), 0, lf->stream, (long long)K, d_status, d_red);
    LF_TRY(lf, hipGetLastError());
    LF_TRY(lf, hipMemcpyAsync(lf->h_out, lf->d_out, back_bytes, hipMemcpyDeviceToHost, lf->stream));
    LF_TRY(lf, hipStreamSynchronize(lf->stream));
    const char *h_out = static_cast<const char *>(lf->h_out);
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
