// rp_score.hip -- librp_score.so: the scorer of include/rp_score.h (MI355X / gfx950).
//
// K given trajectories x n poses against ONE reference path: per pose the curvilinear coordinates (the projection of rp_project /
// rpfe::project, rp_frontend.h, as a batch) and the step's five kinematic checks (ReactivePlanner._check_constraints), per
// trajectory the verdict and the default cost, per call the cheapest feasible trajectory and the counts.  The mapping is the one
// the family shares (rp_check.hip, rp_clearance.hip): a lane is a pose, a wavefront 64 consecutive poses of one trajectory (of the
// flat batch for rp_score_project), a workgroup four wavefronts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_device.h"
#include "rp_frontend.h"
#include "rp_session.h"   // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_score.h"

namespace {

constexpr int SC_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int SC_WAVES = SC_BLOCK / 64;
constexpr int SC_ROW = 16;                      // doubles per segment row (below)
constexpr int SC_LDS_ROWS = 384;                // most segment rows staged in LDS (128 B each, 48 KiB); more: read from device memory
constexpr int SC_FINAL_BLOCK = 1024;            // the one workgroup of rp_score_final_kernel
constexpr uint32_t SC_OUTSIDE = 8u;             // per-pose byte: bits 0..2 the kinematic reason of the step, bit 3 outside the domain

// One row per segment, read by every lane of a wavefront at once (a broadcast from LDS, or a scalar load):
//   [0..1] p0   [2..3] e = p1 - p0   [4..5] t0   [6..7] dt = t1 - t0   [8] pos0   [9] pos1 - pos0   [10] theta0   [11] theta1 - theta0
//   [12..14] the segment's bounding circle cx, cy, r   [15] padding
enum { R_PX, R_PY, R_EX, R_EY, R_TX, R_TY, R_DTX, R_DTY, R_POS, R_DPOS, R_TH, R_DTH, R_CX, R_CY, R_CR };

typedef const double __attribute__((address_space(3))) *lds_cdouble;

// What a lane holds of its best candidate so far: seg < 0 = nothing yet.
struct Held {
    double ad, s, d, lam;
    int32_t seg;
};

// One admissible root of segment k: the candidate's d, and the replacement rule -- STRICTLY smaller |d| only, so that the first
// segment (and on a segment the first root) wins an exact tie.
__device__ __forceinline__ void offer_root(Held &h, double lam, int k, double x, double y, double px, double py, double ex, double ey, double t0x,
                                           double t0y, double dtx, double dty, double pos0, double dpos, double d_limit) {
    if (!(lam >= -1e-12 && lam <= 1.0 + 1e-12)) return;   // (false for NaN)
    lam = fmin(fmax(lam, 0.0), 1.0);
    const double tx = t0x + lam * dtx, ty = t0y + lam * dty, tn = sqrt(tx * tx + ty * ty);
    const double fx = px + lam * ex, fy = py + lam * ey;
    const double dd = (-(x - fx) * ty + (y - fy) * tx) / tn;
    const double ad = fabs(dd);
    if (ad <= d_limit && (h.seg < 0 || ad < h.ad)) { h.ad = ad; h.s = pos0 + lam * dpos; h.d = dd; h.lam = lam; h.seg = k; }
}

// Lower bound in front of the quadratic: the foot point lies on the segment, hence inside its bounding circle (cx, cy, r), and |d|
// is the distance of the point to the foot point -- so |d| >= dist(P, c) - r, and the segment cannot STRICTLY beat the held |d| = m
// (nothing held: cannot stay within m = d_limit) when dist > r + m.  The relative margin keeps rounding of either side from ever
// rejecting a candidate that would have replaced the held one.  False for NaN.
__device__ __forceinline__ bool may_beat(double dist2, double r, double m) { const double s = r + m; return dist2 <= s * s * 1.000001; }

constexpr int SC_LIST = 8;   // open segments a lane lists for itself (below); a wavefront with a longer list walks all segments together

// Both roots of segment k offered to h, in rpfe::project's order.  k may differ from lane to lane.
template <class Row>
__device__ __forceinline__ void offer_segment(Held &h, const Row &row, int k, double x, double y, double d_limit) {
    const double px = row(k, R_PX), py = row(k, R_PY), ex = row(k, R_EX), ey = row(k, R_EY);
    const double t0x = row(k, R_TX), t0y = row(k, R_TY), dtx = row(k, R_DTX), dty = row(k, R_DTY);
    const double pos0 = row(k, R_POS), dpos = row(k, R_DPOS);
    const double qx = x - px, qy = y - py;
    const double a = -(ex * dtx + ey * dty), b = (qx * dtx + qy * dty) - (ex * t0x + ey * t0y), c = qx * t0x + qy * t0y;
    double r0 = __builtin_nan(""), r1 = __builtin_nan("");   // (NaN: no such root)
    if (fabs(a) < 1e-14) {
        if (b != 0.0) r0 = -c / b;
    } else {
        const double disc = b * b - 4.0 * a * c;
        if (disc >= 0.0) {
            const double sq = sqrt(disc);
            const double q = b >= 0.0 ? -0.5 * (b + sq) : -0.5 * (b - sq);
            if (q == 0.0) { r0 = 0.0; r1 = 0.0; }
            else if (b >= 0.0) { r0 = c / q; r1 = q / a; }
            else { r0 = q / a; r1 = c / q; }
        }
    }
    offer_root(h, r0, k, x, y, px, py, ex, ey, t0x, t0y, dtx, dty, pos0, dpos, d_limit);
    offer_root(h, r1, k, x, y, px, py, ex, ey, t0x, t0y, dtx, dty, pos0, dpos, d_limit);
}

// The projection of one pose.  Every lane of the wavefront calls this.
// The plain walk: all segments in ascending order, wave-uniform, a lane skipping what cannot beat what it holds.  The 64 poses of a
// wavefront lie along tens of metres of path, so between them the lanes open most segments and the wavefront pays for every one of
// them.  Hence, unless RP_SCORE_EXHAUSTIVE asks for the plain walk without skipping:
//   1. one cheap uniform pass finds each lane's nearest segment by its circle's centre; the candidates of that segment and its two
//      neighbours give the lane an UPPER bound U on its final |d| (none: U = d_limit) -- the final |d| is the minimum over all candidates;
//   2. a second cheap uniform pass lists, per lane and in ascending order, the segments that may hold a candidate with |d| <= U;
//   3. the lanes then walk their OWN lists side by side, slot by slot.
// Every candidate with |d| <= U is in the list (the segment that gave U included), the list is ascending and a candidate replaces
// the held one only when strictly smaller, so the result is the plain walk's: the first segment that attains the minimum.  Lists
// and plain walk share ONE evaluation site below, so the bits are the same as well.  A wavefront in which some lane has more than
// SC_LIST open segments (far from the path, or outside the domain with d_limit = 20 m) takes the plain walk.
template <bool LDS>
__device__ __forceinline__ Held project_pose(const double *lds_rows, const double *rows, int n_seg, double d_limit, double x, double y, bool want,
                                             bool exhaustive) {
    Held h = {0.0, 0.0, 0.0, 0.0, -1};
    auto row = [&](int k, int q) -> double {
        if constexpr (LDS) return ((lds_cdouble)lds_rows)[k * SC_ROW + q];
        else return ((gcdouble)rows)[(size_t)k * SC_ROW + q];
    };
    int list[SC_LIST], cnt = 0;
    bool lists = false;
    if (!exhaustive) {
        int kn = 0;
        double near2 = __builtin_huge_val();
        for (int k = 0; k < n_seg; ++k) {   // wave-uniform
            const double cx = row(k, R_CX) - x, cy = row(k, R_CY) - y, d2 = cx * cx + cy * cy;
            if (d2 < near2) { near2 = d2; kn = k; }
        }
        Held u = {0.0, 0.0, 0.0, 0.0, -1};
        if (want) {
            offer_segment(u, row, kn, x, y, d_limit);
            if (kn > 0) offer_segment(u, row, kn - 1, x, y, d_limit);
            if (kn + 1 < n_seg) offer_segment(u, row, kn + 1, x, y, d_limit);
        }
        const double bound = u.seg >= 0 ? u.ad : d_limit;
#pragma unroll
        for (int j = 0; j < SC_LIST; ++j) list[j] = 0;
        for (int k = 0; k < n_seg; ++k) {   // wave-uniform
            const double cx = row(k, R_CX) - x, cy = row(k, R_CY) - y;
            if (want && may_beat(cx * cx + cy * cy, row(k, R_CR), bound)) {
#pragma unroll
                for (int j = 0; j < SC_LIST; ++j) list[j] = cnt == j ? k : list[j];
                ++cnt;
            }
        }
        lists = !__any(cnt > SC_LIST);
    }
    const int steps = lists ? SC_LIST : n_seg;
    for (int j = 0; j < steps; ++j) {   // wave-uniform
        int k = j;
        bool open;
        if (lists) {
            open = j < cnt;
#pragma unroll
            for (int q = 0; q < SC_LIST; ++q) k = j == q ? list[q] : k;
        } else {
            const double cx = row(j, R_CX) - x, cy = row(j, R_CY) - y;
            open = want && (exhaustive || may_beat(cx * cx + cy * cy, row(j, R_CR), h.seg < 0 ? d_limit : h.ad));
        }
        if (!__any(open)) {
            if (lists) break;   // (lists are filled from slot 0: nobody has a later slot either)
            continue;
        }
        if (open) offer_segment(h, row, k, x, y, d_limit);
    }
    return h;
}

// make_valid_orientation: into [-pi, pi)
__device__ __forceinline__ double valid_orientation(double a) {
    const double pi = 3.14159265358979323846, two_pi = 2.0 * pi;
    double m = fmod(a, two_pi);
    if (m < 0.0) m += two_pi;
    if (pi <= m && m <= two_pi) m -= two_pi;
    return m;
}

struct ScTable {
    const double *rows;
    int32_t n_seg;
    double d_limit;
};

// what the step's checks read besides the pose arrays
struct ScKin {
    uint32_t mask;
    double dt, wheelbase, a_max, v_switch, v_delta_max, kappa_max;
};

// _check_constraints at step i of one trajectory: the first failing check in the reference's order, or RP_REASON_NONE.  The step
// before is read from memory (prev = the arrays' entry i - 1), never from a neighbour lane.
__device__ __forceinline__ uint32_t step_reason(const ScKin &kin, bool first, double v, double acc, double kappa, double kappa_prev, double theta,
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

// Wavefront w of the grid = chunk w % nchunk of trajectory w / nchunk; lane = pose chunk * 64 + lane.  x .. kappa: [K][n] planes
// (v, a, kappa may be null, theta too for the bare projection).  Outputs, each may be null: s, d, theta_cl [K][n] (NaN outside the
// domain and behind the trajectory's end), segment [K][n] (-1 there), code [K][n] (0 behind the end).
template <bool LDS>
__global__ __launch_bounds__(SC_BLOCK) void rp_score_pose_kernel(ScTable tb, ScKin kin, const double *x, const double *y, const double *theta,
                                                                 const double *v, const double *a, const double *kappa, const int32_t *len, long long K,
                                                                 int n, int nchunk, int exhaustive, double *s_out, double *d_out, double *thcl_out,
                                                                 int32_t *seg_out, uint8_t *code_out) {
    extern __shared__ double sh_rows[];     // n_seg rows (the launch sizes it: a short path leaves room for more workgroups per CU); none if !LDS
    if (LDS) {
        const int nd = tb.n_seg * SC_ROW;   // <= SC_LDS_ROWS * SC_ROW: the host picks this variant and allocates nd doubles
        for (int q = threadIdx.x; q < nd; q += SC_BLOCK) sh_rows[q] = tb.rows[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SC_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= K * nchunk) return;   // (a whole wavefront, behind the only barrier)
    const long long k = w / nchunk;
    const int i = (int)(w % nchunk) * 64 + lane;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    const bool have = i < L;
    const size_t at = (size_t)k * (size_t)n + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never asked
    const double px = x[at], py = y[at];
    const Held h = project_pose<LDS>(sh_rows, tb.rows, tb.n_seg, tb.d_limit, px, py, have, exhaustive != 0);
    if (i >= n) return;
    const size_t out = (size_t)k * (size_t)n + (size_t)i;
    const bool inside = have && h.seg >= 0;
    const double nan = __builtin_nan("");
    if (s_out) s_out[out] = inside ? h.s : nan;
    if (d_out) d_out[out] = inside ? h.d : nan;
    if (seg_out) seg_out[out] = inside ? h.seg : -1;
    if (!theta) return;                        // the bare projection ends here
    const double th = theta[at];
    if (thcl_out) {
        double tcl = nan;
        if (inside) {
            double th0, dth;
            if constexpr (LDS) { th0 = ((lds_cdouble)sh_rows)[h.seg * SC_ROW + R_TH]; dth = ((lds_cdouble)sh_rows)[h.seg * SC_ROW + R_DTH]; }
            else { th0 = tb.rows[(size_t)h.seg * SC_ROW + R_TH]; dth = tb.rows[(size_t)h.seg * SC_ROW + R_DTH]; }
            tcl = valid_orientation(th - (th0 + h.lam * dth));
        }
        thcl_out[out] = tcl;
    }
    if (code_out) {
        uint32_t code = 0;
        if (have) {
            const bool first = i == 0;
            const size_t prev = first ? at : at - 1;
            code = step_reason(kin, first, v ? v[at] : 0.0, a ? a[at] : 0.0, kappa ? kappa[at] : 0.0, kappa ? kappa[prev] : 0.0, th, theta[prev]);
            if (!inside) code |= SC_OUTSIDE;
        }
        code_out[out] = (uint8_t)code;
    }
}

struct ScCost {
    int32_t has_speed, has_s;
    double w_a, desired_speed, desired_d, desired_s;
};

// One wavefront per trajectory, lanes striding over its poses: the first kinematic failure (smallest step; the step's byte holds
// the first failing check), apart from it the first pose outside the domain, and the cost -- every lane adds its poses' terms in
// ascending order, the 64 partial sums meet in a fixed butterfly.  The same result whatever the launch shape.
__global__ __launch_bounds__(SC_BLOCK) void rp_score_traj_kernel(long long K, int n, const int32_t *len, const uint8_t *code, const double *s,
                                                                 const double *d, const double *thcl, const double *v, const double *a, ScCost c,
                                                                 uint32_t *status, double *cost) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (k >= K) return;
    const int L = len ? len[k] : n;
    const size_t base = (size_t)k * (size_t)n;
    const int last = L - 1, mid = L / 2;
    int bad = n, outside = n;   // (above every pose)
    double sum = 0.0;
    for (int i = lane; i < L; i += 64) {   // ascending: a lane keeps its first
        const uint32_t cd = code[base + i];
        if ((cd & 7u) && i < bad) bad = i;
        if ((cd & SC_OUTSIDE) && i < outside) outside = i;
        const double acc = a[base + i], dd = d[base + i], th = fabs(thcl[base + i]);
        double e;
        e = c.w_a * acc; sum += e * e;
        e = 0.25 * (c.desired_d - dd); sum += e * e;
        e = 0.25 * th; sum += e * e;
        if (c.has_speed) { e = 5.0 * (v[base + i] - c.desired_speed); sum += e * e; }
        if (c.has_s) { e = 0.25 * (c.desired_s - s[base + i]); sum += e * e; }
        if (i == last) {
            e = 20.0 * (c.desired_d - dd); sum += e * e;
            e = 5.0 * th; sum += e * e;
            if (c.has_speed) { e = v[base + i] - c.desired_speed; sum += 50.0 * (e * e); }
            if (c.has_s) { e = 20.0 * (c.desired_s - s[base + i]); sum += e * e; }
        }
        if (i == mid && c.has_speed) { e = v[base + i] - c.desired_speed; sum += 100.0 * (e * e); }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int ob = __shfl_xor(bad, off), oo = __shfl_xor(outside, off);
        bad = ob < bad ? ob : bad;
        outside = oo < outside ? oo : outside;
        sum += __shfl_xor(sum, off);
    }
    if (lane == 0) {
        uint32_t reason = RP_REASON_NONE, step = 0;
        if (bad < n) { reason = code[base + bad] & 7u; step = (uint32_t)bad; }
        else if (outside < n) { reason = RP_REASON_OUT_OF_DOMAIN; step = (uint32_t)outside; }
        const bool ok = reason == RP_REASON_NONE;
        step = step > 0xFFFu ? 0xFFFu : step;
        status[k] = ok ? RP_LABEL_FEASIBLE : (RP_LABEL_INFEASIBLE_KINEMATIC | (reason << 4) | (step << 8));
        cost[k] = ok ? sum : __builtin_nan("");
    }
}

// The scalars of a call, by ONE workgroup that strides over the K verdicts (no atomics, nothing to initialise, the same result
// whatever K): red[0] = the k of the lexicographic minimum of (cost, k) over the feasible trajectories (~0: none), red[1] = its
// cost's bits, red[2] = feasible trajectories, red[3 + r] = trajectories with reason r (r = 0 .. 7; 0 counts nothing).
__global__ __launch_bounds__(SC_FINAL_BLOCK) void rp_score_final_kernel(long long K, const uint32_t *status, const double *cost, unsigned long long *red) {
    constexpr int NW = SC_FINAL_BLOCK / 64;
    __shared__ unsigned long long sh_k[NW];
    __shared__ uint32_t sh_cnt[NW][8];   // (K <= RP_SCORE_MAX_POSES = 2^24: a count fits)
    __shared__ double sh_c[NW];
    unsigned long long bestk = ~0ull;
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // cnt[0]: feasible
    double bestc = 0.0;
#pragma unroll 1
    for (long long k = threadIdx.x; k < K; k += SC_FINAL_BLOCK) {   // ascending: a thread keeps the first of equal costs
        const uint32_t st = status[k];
        if (RP_STATUS_LABEL(st) == RP_LABEL_FEASIBLE) {
            ++cnt[0];
            const double cv = cost[k];
            if (cv == cv && (bestk == ~0ull || cv < bestc)) { bestc = cv; bestk = (unsigned long long)k; }
        } else {
            const uint32_t r = RP_STATUS_REASON(st);
#pragma unroll
            for (uint32_t q = 1; q < 8; ++q) cnt[q] += r == q ? 1u : 0u;
        }
    }
    auto merge = [&](unsigned long long ok, double oc) {
        if (ok != ~0ull && (bestk == ~0ull || oc < bestc || (oc == bestc && ok < bestk))) { bestc = oc; bestk = ok; }
    };
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long ok = __shfl_xor(bestk, off);
        const double oc = __shfl_xor(bestc, off);
        merge(ok, oc);
#pragma unroll
        for (int q = 0; q < 8; ++q) cnt[q] += __shfl_xor(cnt[q], off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_k[wave] = bestk; sh_c[wave] = bestc;
#pragma unroll
        for (int q = 0; q < 8; ++q) sh_cnt[wave][q] = cnt[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 1
        for (int w = 1; w < NW; ++w) {
            merge(sh_k[w], sh_c[w]);
#pragma unroll
            for (int q = 0; q < 8; ++q) cnt[q] += sh_cnt[w][q];
        }
        red[0] = bestk;
        red[1] = (unsigned long long)__double_as_longlong(bestc);
        red[2] = cnt[0];
        red[3] = 0ull;
#pragma unroll
        for (int q = 1; q < 8; ++q) red[3 + q] = cnt[q];
    }
}

// rp_score_project's one scalar, by one workgroup: the points whose segment is -1.
__global__ __launch_bounds__(SC_FINAL_BLOCK) void rp_score_outside_kernel(long long n, const int32_t *seg, unsigned long long *red) {
    __shared__ unsigned long long sh[SC_FINAL_BLOCK / 64];
    unsigned long long cnt = 0;
    for (long long i = threadIdx.x; i < n; i += SC_FINAL_BLOCK) cnt += seg[i] < 0 ? 1ull : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SC_FINAL_BLOCK / 64; ++w) cnt += sh[w];
        red[0] = cnt;
    }
}

}  // namespace

struct rp_score : RpSession {
    ScTable tb = {nullptr, 0, 0.0};
    RpTable d_rows;
};

namespace {

// launch of the pose kernel over K trajectories of n poses
void launch_pose(rp_score *sc, const ScKin &kin, const double *x, const double *y, const double *theta, const double *v, const double *a,
                 const double *kappa, const int32_t *len, long long K, int n, bool exhaustive, double *s, double *d, double *thcl, int32_t *seg,
                 uint8_t *code) {
    const int nchunk = (n + 63) / 64;
    const long long waves = K * nchunk;
    const unsigned grid = (unsigned)((waves + SC_WAVES - 1) / SC_WAVES);
    const bool in_lds = sc->tb.n_seg <= SC_LDS_ROWS;
    const auto kernel = in_lds ? rp_score_pose_kernel<true> : rp_score_pose_kernel<false>;
    const size_t lds_bytes = in_lds ? (size_t)sc->tb.n_seg * SC_ROW * sizeof(double) : 0;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(SC_BLOCK), lds_bytes, sc->stream, sc->tb, kin, x, y, theta, v, a, kappa, len, K, n, nchunk, exhaustive ? 1 : 0,
                       s, d, thcl, seg, code);
}

}  // namespace

extern "C" {

int rp_score_abi_version(void) { return RP_SCORE_ABI_VERSION; }

int rp_score_create(rp_score **out, int device) { return session_create(out, device); }

void rp_score_destroy(rp_score *sc) { session_destroy(sc); }

const char *rp_score_last_error(const rp_score *sc) { return session_last_error(sc, "null score object"); }

int rp_score_set_reference(rp_score *sc, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta, double proj_domain_d_limit) {
    if (!sc) return RP_EINVAL;
    if (!sc->stream) return fail(sc, RP_ESTATE, "rp_score_set_reference: the object has no device (rp_score_create failed)");
    if (n < 2 || !ref_xy || !ref_pos || !ref_theta) return fail(sc, RP_EINVAL, "rp_score_set_reference: n < 2 or a null table");
    if (!(proj_domain_d_limit > 0.0) || !std::isfinite(proj_domain_d_limit))
        return fail(sc, RP_EINVAL, "rp_score_set_reference: proj_domain_d_limit must be positive and finite");
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(ref_xy[2 * (size_t)i]) || !std::isfinite(ref_xy[2 * (size_t)i + 1]) || !std::isfinite(ref_pos[i]) || !std::isfinite(ref_theta[i]))
            return fail(sc, RP_EINVAL, "rp_score_set_reference: non-finite value at vertex " + std::to_string(i));
    for (int32_t i = 0; i + 1 < n; ++i) {
        if (!(ref_pos[i + 1] > ref_pos[i])) return fail(sc, RP_EINVAL, "rp_score_set_reference: ref_pos is not strictly increasing at vertex " + std::to_string(i + 1));
        if (ref_xy[2 * (size_t)i] == ref_xy[2 * (size_t)i + 2] && ref_xy[2 * (size_t)i + 1] == ref_xy[2 * (size_t)i + 3])
            return fail(sc, RP_EINVAL, "rp_score_set_reference: zero-length segment " + std::to_string(i));
    }
    std::vector<double> rows;
    std::vector<rpfe::Pt> ref, tan;
    try {
        ref.resize(n);
        for (int32_t i = 0; i < n; ++i) ref[i] = {ref_xy[2 * (size_t)i], ref_xy[2 * (size_t)i + 1]};
        tan = rpfe::vertex_tangents(ref);
        rows.assign((size_t)(n - 1) * SC_ROW, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(sc, RP_ENOMEM, "rp_score_set_reference: host memory");
    }
    for (int32_t k = 0; k + 1 < n; ++k) {
        double *r = rows.data() + (size_t)k * SC_ROW;
        const double ex = ref[k + 1].x - ref[k].x, ey = ref[k + 1].y - ref[k].y;
        r[R_PX] = ref[k].x; r[R_PY] = ref[k].y; r[R_EX] = ex; r[R_EY] = ey;
        r[R_TX] = tan[k].x; r[R_TY] = tan[k].y; r[R_DTX] = tan[k + 1].x - tan[k].x; r[R_DTY] = tan[k + 1].y - tan[k].y;
        r[R_POS] = ref_pos[k]; r[R_DPOS] = ref_pos[k + 1] - ref_pos[k];
        r[R_TH] = ref_theta[k]; r[R_DTH] = ref_theta[k + 1] - ref_theta[k];
        r[R_CX] = ref[k].x + 0.5 * ex; r[R_CY] = ref[k].y + 0.5 * ey;
        r[R_CR] = 0.5 * std::sqrt(ex * ex + ey * ey) * (1.0 + 1e-12);   // (rounded up: the circle holds both end points)
        for (int q = 0; q < SC_ROW; ++q)
            if (!std::isfinite(r[q])) return fail(sc, RP_EINVAL, "rp_score_set_reference: segment " + std::to_string(k) + " is not finite");
    }
    const int rc = replace_tables(sc, {{&sc->d_rows, &rows}});
    if (rc != RP_OK) return rc;
    sc->tb = {sc->d_rows.p, n - 1, proj_domain_d_limit};
    return RP_OK;
}

int rp_score_project(rp_score *sc, int64_t n_points, const double *x, const double *y, double *s, double *d, int32_t *segment, int64_t *n_outside) {
    if (!sc) return RP_EINVAL;
    if (n_points < 0 || n_points > RP_SCORE_MAX_POSES) return fail(sc, RP_EINVAL, "rp_score_project: n_points < 0 or beyond RP_SCORE_MAX_POSES");
    if (n_points > 0 && (!x || !y)) return fail(sc, RP_EINVAL, "rp_score_project: null points");
    if (!sc->stream) return fail(sc, RP_ESTATE, "rp_score_project: the object has no device (rp_score_create failed)");
    if (!sc->tb.rows) return fail(sc, RP_ESTATE, "rp_score_project: no reference set (rp_score_set_reference)");
    if (n_points == 0) {
        if (n_outside) *n_outside = 0;
        return RP_OK;
    }
    RP_TRY(sc, hipSetDevice(sc->device));
    const size_t P = (size_t)n_points;
    const size_t in_bytes = 2 * P * sizeof(double);
    // results on the device: scalar | s [P] | d [P] | segment [P]
    const size_t s_off = 8 * sizeof(unsigned long long), d_off = s_off + P * sizeof(double), seg_off = d_off + P * sizeof(double);
    const size_t out_bytes = seg_off + P * sizeof(int32_t);
    const int rc = grow_call(sc, "rp_score", in_bytes, out_bytes, out_bytes);
    if (rc != RP_OK) return rc;
    double *h_in = static_cast<double *>(sc->h_in.p);
    std::memcpy(h_in, x, P * sizeof(double));
    std::memcpy(h_in + P, y, P * sizeof(double));
    RP_TRY(sc, hipMemcpyAsync(sc->d_in.p, sc->h_in.p, in_bytes, hipMemcpyHostToDevice, sc->stream));
    const double *d_x = static_cast<const double *>(sc->d_in.p);
    char *d_out = static_cast<char *>(sc->d_out.p);
    int32_t *d_seg = reinterpret_cast<int32_t *>(d_out + seg_off);
    const ScKin kin = {0u, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
    // the flat batch as ONE trajectory of n_points poses: wavefront w = points 64 w .. 64 w + 63
    launch_pose(sc, kin, d_x, d_x + P, nullptr, nullptr, nullptr, nullptr, nullptr, 1, (int)n_points, false, reinterpret_cast<double *>(d_out + s_off),
                reinterpret_cast<double *>(d_out + d_off), nullptr, d_seg, nullptr);
    RP_TRY(sc, hipGetLastError());
    hipLaunchKernelGGL(rp_score_outside_kernel, dim3(1), dim3(SC_FINAL_BLOCK), 0, sc->stream, (long long)n_points, d_seg,
                       reinterpret_cast<unsigned long long *>(d_out));
    RP_TRY(sc, hipGetLastError());
    RP_TRY(sc, hipMemcpyAsync(sc->h_out.p, sc->d_out.p, out_bytes, hipMemcpyDeviceToHost, sc->stream));
    RP_TRY(sc, hipStreamSynchronize(sc->stream));
    const char *h_out = static_cast<const char *>(sc->h_out.p);
    if (n_outside) *n_outside = (int64_t) * reinterpret_cast<const unsigned long long *>(h_out);
    if (s) std::memcpy(s, h_out + s_off, P * sizeof(double));
    if (d) std::memcpy(d, h_out + d_off, P * sizeof(double));
    if (segment) std::memcpy(segment, h_out + seg_off, P * sizeof(int32_t));
    return RP_OK;
}

int rp_score_evaluate(rp_score *sc, const rp_params *p, const rp_cost *cost, int64_t K, int32_t n_poses, const double *x, const double *y,
                      const double *theta, const double *v, const double *a, const double *kappa, const int32_t *len, uint32_t flags, double *s_out,
                      double *d_out, double *theta_cl_out, uint32_t *status, double *cost_out, int64_t *best, double *best_cost, int64_t *n_feasible,
                      int64_t *reason_counts) {
    if (!sc) return RP_EINVAL;
    if (!p || !cost) return fail(sc, RP_EINVAL, "rp_score_evaluate: null params or cost");
    if (p->struct_size != sizeof(rp_params)) return fail(sc, RP_EABI, "rp_score_evaluate: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (cost->struct_size != sizeof(rp_cost)) return fail(sc, RP_EABI, "rp_score_evaluate: rp_cost.struct_size is not this library's sizeof(rp_cost)");
    if (K < 0 || n_poses < 1) return fail(sc, RP_EINVAL, "rp_score_evaluate: K < 0 or n_poses < 1");
    if (K > RP_SCORE_MAX_POSES || K * (int64_t)n_poses > RP_SCORE_MAX_POSES)
        return fail(sc, RP_EINVAL, "rp_score_evaluate: K * n_poses beyond RP_SCORE_MAX_POSES");
    if (flags & ~(uint32_t)RP_SCORE_EXHAUSTIVE) return fail(sc, RP_EINVAL, "rp_score_evaluate: unknown flags");
    if (cost->kind != RP_COST_DEFAULT && cost->kind != RP_COST_FAILSAFE)
        return fail(sc, RP_EINVAL, "rp_score_evaluate: cost kind must be RP_COST_DEFAULT or RP_COST_FAILSAFE");
    const double desired[3] = {cost->desired_speed, cost->desired_d, cost->desired_s};
    for (double q : desired)
        if (!std::isnan(q) && !std::isfinite(q)) return fail(sc, RP_EINVAL, "rp_score_evaluate: a desired value of the cost is infinite");
    if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return fail(sc, RP_EINVAL, "rp_score_evaluate: dt must be positive");
    if (K > 0 && (!x || !y || !theta)) return fail(sc, RP_EINVAL, "rp_score_evaluate: null poses");
    const uint32_t cm = p->constraint_mask;
    const bool failsafe = cost->kind == RP_COST_FAILSAFE;
    const bool has_speed = !failsafe && !std::isnan(cost->desired_speed), has_s = !failsafe && !std::isnan(cost->desired_s);
    if (K > 0) {
        if ((cm & (RP_CHECK_VELOCITY | RP_CHECK_YAW_RATE | RP_CHECK_ACCELERATION)) && !v)
            return fail(sc, RP_EINVAL, "rp_score_evaluate: constraint_mask asks for a check that reads v, and v is NULL");
        if ((cm & (RP_CHECK_KAPPA | RP_CHECK_KAPPA_DOT)) && !kappa)
            return fail(sc, RP_EINVAL, "rp_score_evaluate: constraint_mask asks for a check that reads kappa, and kappa is NULL");
        if (!a) return fail(sc, RP_EINVAL, "rp_score_evaluate: a is NULL (the cost's acceleration term reads it)");
        if (has_speed && !v) return fail(sc, RP_EINVAL, "rp_score_evaluate: desired_speed is set and v is NULL");
    }
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(sc, RP_EINVAL, "rp_score_evaluate: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (!sc->stream) return fail(sc, RP_ESTATE, "rp_score_evaluate: the object has no device (rp_score_create failed)");
    if (!sc->tb.rows) return fail(sc, RP_ESTATE, "rp_score_evaluate: no reference set (rp_score_set_reference)");
    if (K == 0) {
        if (best) *best = -1;
        if (best_cost) *best_cost = std::nan("");
        if (n_feasible) *n_feasible = 0;
        if (reason_counts) std::memset(reason_counts, 0, 8 * sizeof(int64_t));
        return RP_OK;
    }
    RP_TRY(sc, hipSetDevice(sc->device));
    const size_t P = (size_t)K * (size_t)n_poses, Kz = (size_t)K;
    // inputs: x | y | theta | a | v? | kappa? | len?
    const int n_planes = 4 + (v ? 1 : 0) + (kappa ? 1 : 0);
    const size_t in_bytes = (size_t)n_planes * P * sizeof(double) + (len ? Kz * sizeof(int32_t) : 0);
    // results on the device: scalars | cost [K] | status [K] | (8-byte aligned) s [P] | d [P] | theta_cl [P] | code [P]; a call copies back
    // the front of it, as far as it asks for
    const size_t cost_off = 16 * sizeof(unsigned long long), st_off = cost_off + Kz * sizeof(double);
    const size_t s_off = align8(st_off + Kz * sizeof(uint32_t)), d_off = s_off + P * sizeof(double), th_off = d_off + P * sizeof(double);
    const size_t code_off = th_off + P * sizeof(double);
    const size_t dev_bytes = code_off + P;
    const size_t back_bytes = theta_cl_out ? code_off : d_out ? th_off : s_out ? d_off : s_off;
    const int rc = grow_call(sc, "rp_score", in_bytes, back_bytes, dev_bytes);
    if (rc != RP_OK) return rc;
    double *h_in = static_cast<double *>(sc->h_in.p);
    const double *d_in = static_cast<const double *>(sc->d_in.p);
    int plane = 0;
    auto put = [&](const double *src) -> const double * {
        if (!src) return nullptr;
        std::memcpy(h_in + (size_t)plane * P, src, P * sizeof(double));
        return d_in + (size_t)(plane++) * P;
    };
    const double *d_x = put(x), *d_y = put(y), *d_th = put(theta), *d_a = put(a), *d_v = put(v), *d_kappa = put(kappa);
    const int32_t *d_len = nullptr;
    if (len) {
        std::memcpy(h_in + (size_t)plane * P, len, Kz * sizeof(int32_t));
        d_len = reinterpret_cast<const int32_t *>(d_in + (size_t)plane * P);
    }
    RP_TRY(sc, hipMemcpyAsync(sc->d_in.p, sc->h_in.p, in_bytes, hipMemcpyHostToDevice, sc->stream));
    char *dv = static_cast<char *>(sc->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(dv);
    double *d_cost = reinterpret_cast<double *>(dv + cost_off), *d_s = reinterpret_cast<double *>(dv + s_off);
    double *d_d = reinterpret_cast<double *>(dv + d_off), *d_thcl = reinterpret_cast<double *>(dv + th_off);
    uint32_t *d_status = reinterpret_cast<uint32_t *>(dv + st_off);
    uint8_t *d_code = reinterpret_cast<uint8_t *>(dv + code_off);
    const ScKin kin = {cm, p->dt, p->wheelbase, p->a_max, p->v_switch, p->v_delta_max, std::tan(p->delta_max) / p->wheelbase};
    launch_pose(sc, kin, d_x, d_y, d_th, d_v, d_a, d_kappa, d_len, (long long)K, (int)n_poses, (flags & RP_SCORE_EXHAUSTIVE) != 0, d_s, d_d, d_thcl, nullptr,
                d_code);
    RP_TRY(sc, hipGetLastError());
    // cost_function.py:82-92: the fail-safe cost is the default one with w_a = 1, desired_d = 0 and no v / s terms
    const ScCost cc = {has_speed ? 1 : 0, has_s ? 1 : 0, failsafe ? 1.0 : cost->w_a, has_speed ? cost->desired_speed : 0.0, failsafe ? 0.0 : cost->desired_d,
                       has_s ? cost->desired_s : 0.0};
    hipLaunchKernelGGL(rp_score_traj_kernel, dim3((unsigned)((K + SC_WAVES - 1) / SC_WAVES)), dim3(SC_BLOCK), 0, sc->stream, (long long)K, (int)n_poses, d_len,
                       d_code, d_s, d_d, d_thcl, d_v, d_a, cc, d_status, d_cost);
    RP_TRY(sc, hipGetLastError());
    hipLaunchKernelGGL(rp_score_final_kernel, dim3(1), dim3(SC_FINAL_BLOCK), 0, sc->stream, (long long)K, d_status, d_cost, d_red);
    RP_TRY(sc, hipGetLastError());
    RP_TRY(sc, hipMemcpyAsync(sc->h_out.p, sc->d_out.p, back_bytes, hipMemcpyDeviceToHost, sc->stream));
    RP_TRY(sc, hipStreamSynchronize(sc->stream));
    const char *h_out = static_cast<const char *>(sc->h_out.p);
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    const bool any = h_red[0] < (unsigned long long)K;
    if (best) *best = any ? (int64_t)h_red[0] : -1;
    if (best_cost) {
        if (any) std::memcpy(best_cost, &h_red[1], sizeof(double));
        else *best_cost = std::nan("");
    }
    if (n_feasible) *n_feasible = (int64_t)h_red[2];
    if (reason_counts)
        for (int q = 0; q < 8; ++q) reason_counts[q] = (int64_t)h_red[3 + q];
    if (cost_out) std::memcpy(cost_out, h_out + cost_off, Kz * sizeof(double));
    if (status) std::memcpy(status, h_out + st_off, Kz * sizeof(uint32_t));
    if (s_out) std::memcpy(s_out, h_out + s_off, P * sizeof(double));
    if (d_out) std::memcpy(d_out, h_out + d_off, P * sizeof(double));
    if (theta_cl_out) std::memcpy(theta_cl_out, h_out + th_off, P * sizeof(double));
    return RP_OK;
}

}  // extern "C"
