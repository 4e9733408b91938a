// rp_check_rules.h -- the obstacle walk of include/rp_check.h, stated once: the layout of the obstacle tables and their builder,
// cc.collide of one rectangle against them, and both tests of one 64-pose chunk of a trajectory.  Included by rp_check.hip
// (librp_check.so) and by rp_pick.hip (librp_pick.so); everything here has internal linkage, nothing of it is exported by either.
#ifndef RP_CHECK_RULES_H
#define RP_CHECK_RULES_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "rp_device.h"
#include "../../include/rp_check.h"

namespace {

constexpr int CK_ROW = 10;                      // doubles per static row (below)
constexpr int32_t CK_NONE = 0x7f7f7f7f;         // "no hit yet" of the first-hit arrays (a byte fill), above every pose index

// Static shapes as ONE table, rectangles first, then triangles, then circles; every lane of a wavefront reads the same row
// (a broadcast from LDS, or a scalar load).  Row: [0..5] the shape -- rectangle cx, cy, ux, uy, hl, hw | triangle x1 .. y3 |
// circle cx, cy, r -- then [6..8] its bounding circle cx, cy, r and one double of padding.
// Dynamic rectangles: struct-of-arrays planes [7][n_dyn][n_steps] cx, cy, ux, uy, hl, hw, r_bound (cx = NaN: absent), so that the
// lanes of a wavefront -- consecutive time indices -- read consecutive addresses.
struct CkTables {
    const double *stat;
    const double *dyn;
    int32_t n_sobb, n_tri, n_circ, n_dyn, n_steps, dyn_t0;
};

typedef const double __attribute__((address_space(3))) *lds_cdouble;

// cc.collide(rectangle e at scenario time index t) for the lanes that `want` it.  Every lane of the wavefront calls this.
// r: radius of a circle around e (bounding-circle rejection in front of every exact test; the small relative margin keeps it from
// rejecting a pair the exact test would accept).  A lane stops at its first hit.
template <bool LDS>
__device__ __forceinline__ bool ck_collides(const CkTables &tb, const double *lds_rows, const Obb &e, double r, long long t, bool want) {
    bool hit = false;
    auto row = [&](int j, int q) -> double {
        if constexpr (LDS) return ((lds_cdouble)lds_rows)[j * CK_ROW + q];
        else return ((gcdouble)tb.stat)[(size_t)j * CK_ROW + q];
    };
    const int n_static = tb.n_sobb + tb.n_tri + tb.n_circ;
    for (int j = 0; j < n_static; ++j) {   // wave-uniform
        const double dx = row(j, 6) - e.cx, dy = row(j, 7) - e.cy, rr = r + row(j, 8);
        if (want && !hit && dx * dx + dy * dy <= rr * rr * 1.000001) {   // false for NaN
            if (j < tb.n_sobb) {
                const Obb b = {row(j, 0), row(j, 1), row(j, 2), row(j, 3), row(j, 4), row(j, 5)};
                hit = obb_obb(e, b);
            } else if (j < tb.n_sobb + tb.n_tri) {
                const double tv[6] = {row(j, 0), row(j, 1), row(j, 2), row(j, 3), row(j, 4), row(j, 5)};
                hit = obb_tri(e, tv);
            } else {
                hit = obb_circ(e, row(j, 0), row(j, 1), row(j, 2));
            }
        }
    }
    // dynamic rectangles at the lane's own time index; outside the table: absent
    const long long k = t - (long long)tb.dyn_t0;
    const bool in_table = want && k >= 0 && k < (long long)tb.n_steps;
    const size_t kc = in_table ? (size_t)k : 0;
    const size_t plane = (size_t)tb.n_dyn * (size_t)tb.n_steps;
    const gcdouble dyn = (gcdouble)tb.dyn;
    for (int j = 0; j < tb.n_dyn; ++j) {
        const bool open = in_table && !hit;
        if (!__any(open)) break;   // the wavefront goes on while any lane is unresolved
        const gcdouble o = dyn + (size_t)j * (size_t)tb.n_steps + kc;
        const double cx = o[0], cy = o[plane], rr = r + o[6 * plane];
        const double dx = cx - e.cx, dy = cy - e.cy;
        if (open && dx * dx + dy * dy <= rr * rr * 1.000001) {   // false for NaN: absent
            const Obb b = {cx, cy, o[2 * plane], o[3 * plane], o[4 * plane], o[5 * plane]};
            hit = obb_obb(e, b);
        }
    }
    return hit;
}

// the ego rectangle of the pose at poses[at]: planes x | y | theta with stride plane
__device__ __forceinline__ Obb ck_ego(const double *poses, size_t plane, size_t at, double wb_rear_axle, double hl, double hw) {
    double s, c;
    sincos(poses[2 * plane + at], &s, &c);
    return {poses[at] + wb_rear_axle * c, poses[plane + at] + wb_rear_axle * s, c, s, hl, hw};
}

// RP_TRAJ_POSES for the lane's pose i (the lanes that `have` one), at scenario time index t0 + i * factor
template <bool LDS>
__device__ __forceinline__ bool ck_pose_hit(const CkTables &tb, const double *lds_rows, const Obb &ego, double hl, double hw, int t0, int factor, int i, bool have) {
    return ck_collides<LDS>(tb, lds_rows, ego, sqrt(hl * hl + hw * hw), (long long)t0 + (long long)i * factor, have);
}

// RP_TRAJ_SWEPT for the segment that starts at the lane's pose i (i + 1 < L), at scenario time index t0 + i: the rectangle of pose
// i + 1 comes from the next lane; the wavefront's last lane loads that pose itself
template <bool LDS>
__device__ __forceinline__ bool ck_segment_hit(const CkTables &tb, const double *lds_rows, const Obb &ego, const double *poses, size_t plane, size_t at,
                                               double wb_rear_axle, double hl, double hw, int t0, int i, int L, int lane) {
    const bool seg = i + 1 < L;
    Obb nxt = {__shfl_down(ego.cx, 1), __shfl_down(ego.cy, 1), __shfl_down(ego.ux, 1), __shfl_down(ego.uy, 1), hl, hw};
    if (lane == 63 && seg) {
        double s1, c1;
        sincos(poses[2 * plane + at + 1], &s1, &c1);
        nxt.cx = poses[at + 1] + wb_rear_axle * c1; nxt.cy = poses[plane + at + 1] + wb_rear_axle * s1; nxt.ux = c1; nxt.uy = s1;
    }
    const Obb m = merge_swept(ego, seg ? nxt : ego);
    return ck_collides<LDS>(tb, lds_rows, m, sqrt(m.hl * m.hl + m.hw * m.hw), (long long)t0 + (long long)i, seg);
}

// ---- host: rp_checker_set_obstacles' refusals and its two tables -----------------------------------------------------------------
// RP_OK, the static rows `a` and the dynamic planes `e`, or the code (RP_EINVAL, RP_ENOMEM) and the message behind `who: `.
inline int ck_build_tables(const char *who, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ,
                           int32_t n_dyn, int32_t n_steps, const double *dyn, std::vector<double> &a, std::vector<double> &e, std::string &msg) {
    const std::string w = std::string(who) + ": ";
    if (n_sobb < 0 || n_tri < 0 || n_circ < 0 || n_dyn < 0 || n_steps < 0 || (n_sobb && !sobb) || (n_tri && !tri) || (n_circ && !circ) ||
        (n_dyn && n_steps && !dyn)) {
        msg = w + "negative count or null table";
        return RP_EINVAL;
    }
    if ((int64_t)n_sobb + n_tri + n_circ > INT32_MAX / CK_ROW) { msg = w + "too many static shapes"; return RP_EINVAL; }
    try {
        a.assign(((size_t)n_sobb + (size_t)n_tri + (size_t)n_circ) * CK_ROW, 0.0);
        e.assign((size_t)7 * (size_t)n_dyn * (size_t)n_steps, 0.0);
    } catch (const std::bad_alloc &) {
        msg = w + "host memory";
        return RP_ENOMEM;
    }
    double *r = a.data();
    for (int j = 0; j < n_sobb; ++j, r += CK_ROW) {   // (ux, uy from the host's cos / sin, as rp_set_obstacles)
        const double *o = sobb + 5 * (size_t)j;
        r[0] = o[0]; r[1] = o[1]; r[2] = std::cos(o[2]); r[3] = std::sin(o[2]); r[4] = o[3]; r[5] = o[4];
        r[6] = o[0]; r[7] = o[1]; r[8] = std::sqrt(o[3] * o[3] + o[4] * o[4]);
    }
    for (int j = 0; j < n_tri; ++j, r += CK_ROW) {
        const double *o = tri + 6 * (size_t)j;
        for (int q = 0; q < 6; ++q) r[q] = o[q];
        const double bx = (o[0] + o[2] + o[4]) / 3.0, by = (o[1] + o[3] + o[5]) / 3.0;
        double rr = 0.0;
        for (int q = 0; q < 3; ++q) rr = std::fmax(rr, std::hypot(o[2 * q] - bx, o[2 * q + 1] - by));
        r[6] = bx; r[7] = by; r[8] = rr;
    }
    for (int j = 0; j < n_circ; ++j, r += CK_ROW) {
        const double *o = circ + 3 * (size_t)j;
        r[0] = o[0]; r[1] = o[1]; r[2] = o[2];
        r[6] = o[0]; r[7] = o[1]; r[8] = o[2];
    }
    const size_t plane = (size_t)n_dyn * (size_t)n_steps;
    for (size_t at = 0; at < plane; ++at) {
        const double *o = dyn + 5 * at;
        e[at] = o[0]; e[plane + at] = o[1];
        e[2 * plane + at] = std::cos(o[2]); e[3 * plane + at] = std::sin(o[2]);
        e[4 * plane + at] = o[3]; e[5 * plane + at] = o[4];
        e[6 * plane + at] = std::sqrt(o[3] * o[3] + o[4] * o[4]);
    }
    return RP_OK;
}

}  // namespace

#endif  // RP_CHECK_RULES_H
