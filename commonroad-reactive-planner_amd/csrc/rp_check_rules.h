// rp_check_rules.h -- the obstacle walk of include/rp_check.h, stated once: the obstacle tables as the kernels see them, cc.collide
// of one rectangle against them, and both tests of one 64-pose chunk of a trajectory.  The tables' host builder is
// rp_obstacle_tables.h, included here.  Everything here has internal linkage, nothing of it is exported by a library that includes it.
#ifndef RP_CHECK_RULES_H
#define RP_CHECK_RULES_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "rp_device.h"
#include "rp_obstacle_tables.h"
#include "../../include/rp_check.h"

namespace {

constexpr int CK_ROW = OT_ROW;                  // doubles per static row (rp_obstacle_tables.h)
constexpr int32_t CK_NONE = 0x7f7f7f7f;         // "no hit yet" of the first-hit arrays (a byte fill), above every pose index

// The tables of rp_obstacle_tables.h.  Every lane of a wavefront reads the same static row (a broadcast from LDS, or a scalar load);
// the dynamic planes are laid out so that the lanes of a wavefront -- consecutive time indices -- read consecutive addresses.
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

}  // namespace

#endif  // RP_CHECK_RULES_H
