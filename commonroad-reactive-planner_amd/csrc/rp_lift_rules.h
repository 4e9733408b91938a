// rp_lift_rules.h -- the per-pose lift step of include/rp_lift.h, stated once: the segment row and its host builder, the segment
// search, the step's five kinematic checks and the verdict word.  The walk of a trajectory that applies them, 64 poses at a time, is
// the text of rp_lift_walk.inc.  Included by rp_lift.hip (librp_lift.so) and by rp_pick.hip (librp_pick.so); everything here has
// internal linkage, nothing of it is exported by either library.
#ifndef RP_LIFT_RULES_H
#define RP_LIFT_RULES_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "rp_device.h"
#include "rp_frontend.h"
#include "../../include/rp_amd.h"

namespace {

constexpr int LF_ROW = 16;                      // doubles per segment row (below)
constexpr int LF_PLANES = 8;                    // x, y, theta, v, a, kappa, kappa_dot, theta_cl
constexpr uint32_t LF_KEY_NONE = 0xFFFFFFFFu;   // a trajectory's verdict key (below): nothing failed
constexpr uint32_t LF_KEY_LATE = 0x40000000u;   // ... |d| beyond the limit: behind every step's own failure

// One row per segment:
//   [0..1] p0   [2..3] e = p1 - p0   [4..5] t0   [6..7] dt = t1 - t0   [8] pos0   [9] pos1 - pos0   [10] theta0   [11] theta1 - theta0
//   [12] curv0   [13] curv1 - curv0   [14] curv_d0   [15] curv_d1 - curv_d0
enum { R_PX, R_PY, R_EX, R_EY, R_TX, R_TY, R_DTX, R_DTY, R_POS, R_DPOS, R_TH, R_DTH, R_KR, R_DKR, R_KRD, R_DKRD };

typedef const double __attribute__((address_space(3))) *lf_lds_cdouble;

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
        if constexpr (LDS) return ((lf_lds_cdouble)lds)[k * LF_ROW + q];
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

// The wavefront's verdict from its lanes' keys: every lane returns the status word.
__device__ __forceinline__ uint32_t lf_verdict(uint32_t best) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t ob = __shfl_xor(best, o);
        best = ob < best ? ob : best;
    }
    uint32_t st = RP_LABEL_FEASIBLE;
    if (best != LF_KEY_NONE) {
        uint32_t step = (best & ~LF_KEY_LATE) >> 3;
        step = step > 0xFFFu ? 0xFFFu : step;
        st = RP_LABEL_INFEASIBLE_KINEMATIC | ((best & 7u) << 4) | (step << 8);
    }
    return st;
}

// ---- host: rp_lift_set_reference's refusals and its rows --------------------------------------------------------------------------
// RP_OK and the n - 1 rows, or the code (RP_EINVAL, RP_ENOMEM) and the message behind `who: `.
inline int lf_build_rows(const char *who, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta, const double *ref_curv,
                         const double *ref_curv_d, double proj_domain_d_limit, std::vector<double> &rows, std::string &msg) {
    const std::string w = std::string(who) + ": ";
    if (n < 2 || !ref_xy || !ref_pos || !ref_theta || !ref_curv || !ref_curv_d) { msg = w + "n < 2 or a null table"; return RP_EINVAL; }
    if (!(proj_domain_d_limit > 0.0) || !std::isfinite(proj_domain_d_limit)) { msg = w + "proj_domain_d_limit must be positive and finite"; return RP_EINVAL; }
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(ref_xy[2 * (size_t)i]) || !std::isfinite(ref_xy[2 * (size_t)i + 1]) || !std::isfinite(ref_pos[i]) || !std::isfinite(ref_theta[i]) ||
            !std::isfinite(ref_curv[i]) || !std::isfinite(ref_curv_d[i])) {
            msg = w + "non-finite value at vertex " + std::to_string(i);
            return RP_EINVAL;
        }
    for (int32_t i = 0; i + 1 < n; ++i) {
        if (!(ref_pos[i + 1] > ref_pos[i])) { msg = w + "ref_pos is not strictly increasing at vertex " + std::to_string(i + 1); return RP_EINVAL; }
        if (ref_xy[2 * (size_t)i] == ref_xy[2 * (size_t)i + 2] && ref_xy[2 * (size_t)i + 1] == ref_xy[2 * (size_t)i + 3]) {
            msg = w + "zero-length segment " + std::to_string(i);
            return RP_EINVAL;
        }
    }
    std::vector<rpfe::Pt> ref, tan;
    try {
        ref.resize(n);
        for (int32_t i = 0; i < n; ++i) ref[i] = {ref_xy[2 * (size_t)i], ref_xy[2 * (size_t)i + 1]};
        tan = rpfe::vertex_tangents(ref);
        rows.assign((size_t)(n - 1) * LF_ROW, 0.0);
    } catch (const std::bad_alloc &) {
        msg = w + "host memory";
        return RP_ENOMEM;
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
            if (!std::isfinite(r[q])) { msg = w + "segment " + std::to_string(k) + " is not finite"; return RP_EINVAL; }
    }
    return RP_OK;
}

// trips of the segment search over n vertices: n = n_seg + 1 possible answers
inline int32_t lf_search_iters(int32_t n) {
    int32_t iters = 0;
    while (((int64_t)1 << iters) < (int64_t)n) ++iters;
    return iters;
}

}  // namespace

#endif  // RP_LIFT_RULES_H
