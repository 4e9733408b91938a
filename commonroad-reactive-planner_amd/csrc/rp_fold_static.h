// A few static rectangles checked as rows of the dynamic-obstacle table ("fold_static", rp_host.hip).
//
// The evaluation kernels answer the collision query against static shapes through a grid lookup per pose, a wave-wide OR of the
// lanes' cluster masks and a walk over cluster descriptors and shape rows (rp_device.h: pose_collides, the COLL = 2 instances);
// against dynamic obstacles through the (pair, step) masks of the profile and a walk over the rows of the obstacles near a pose
// (COLL = 1).  For a rectangle both end in the same four separating axes on the same six numbers (obb_sep_on_a_axes,
// obb_sep_on_b_axes), and what stands in front of them is a conservative superset either way.  A scene with a handful of parked
// vehicles and no road boundary therefore need not carry the static machinery at all: its rectangles become obstacles of the dynamic
// table whose row is the same at every step, and every launch of the plan takes the COLL = 1 instance.
//
// This header builds that table on the host and decides whether a set of tables may be folded.  Plain C++: no HIP, so that
// tests/test_fold_static_table.py compiles it into a host library on a box without a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace rpfs {

// rows of the static rectangles as rp_set_obstacles lays them out (rp_device.h: OB_ROW): cx, cy, ux, uy, hl, hw, r_bound, -
constexpr int kRectRow = 8;
// The widest mask without the overflow path of pose_collides: bits 0 .. 62 (bit 63 stands for "obstacle 63 and all behind it").
constexpr int kMaxObstacles = 63;
// Steps a folded table may cover: 63 obstacles x 9 doubles x 8192 steps = 37 MB at the very most.  A plan further out than that
// from the dynamic table's first step keeps the unfolded tables.
constexpr int kMaxSteps = 8192;
// Steps added behind the last one asked for when the table is (re)built, so that a replanning loop -- whose time_step0 advances by
// one per cycle -- rebuilds it once in kHeadroom cycles and not in every one.
constexpr int kHeadroom = 128;

// layout of the dynamic table (the same arithmetic as rp_device.h: dyn_xy_offset, dyn_rmax_offset, dyn_table_doubles; rp_host.hip
// checks that they agree before it uploads a folded table)
inline size_t xy_offset(int n, int steps) { return ((size_t)7 * (size_t)n * (size_t)steps + 1) & ~(size_t)1; }
inline size_t rmax_offset(int n, int steps) { return xy_offset(n, steps) + (size_t)2 * (size_t)n * (size_t)steps; }
inline size_t table_doubles(int n, int steps) { return rmax_offset(n, steps) + (size_t)n; }

enum Refusal {
    kFoldOk = 0,
    kNoRectangle,      // nothing to fold
    kTriangle,         // a triangle present
    kCircle,           // a circle present
    kTooManyRects,     // more rectangles than the threshold
    kTooManyTotal,     // n_dyn + n_sobb > 63: a mask would take the overflow path
    kRadius,           // a rectangle larger than every dynamic obstacle: the pre-test radius of pose_collides would grow
    kNonFinite,        // a rectangle row (or the dynamic table's largest radius) that is not finite
};

// May these tables be folded?  `rects`: [n_sobb][kRectRow]; `dyn_rmax_all`: largest bounding radius of a dynamic obstacle at any
// step (ignored when n_dyn == 0: the folded table then holds the rectangles alone and its radius is the largest rectangle's).
inline int refusal(int n_sobb, const double *rects, int n_tri, int n_circ, int n_dyn, double dyn_rmax_all, int max_rects) {
    if (n_tri > 0) return kTriangle;
    if (n_circ > 0) return kCircle;
    if (n_sobb <= 0) return kNoRectangle;
    if (n_sobb > max_rects) return kTooManyRects;
    if ((long long)n_dyn + (long long)n_sobb > kMaxObstacles) return kTooManyTotal;
    for (int j = 0; j < n_sobb; ++j)
        for (int q = 0; q < 7; ++q)
            if (!std::isfinite(rects[(size_t)j * kRectRow + q])) return kNonFinite;
    if (n_dyn > 0) {
        if (!std::isfinite(dyn_rmax_all)) return kNonFinite;
        for (int j = 0; j < n_sobb; ++j)
            if (rects[(size_t)j * kRectRow + 6] > dyn_rmax_all) return kRadius;
    }
    return kFoldOk;
}

// The bounding radius the folded view hands to the kernels (ObsTables::dyn_rmax_all).
inline double folded_rmax_all(int n_sobb, const double *rects, int n_dyn, double dyn_rmax_all) {
    if (n_dyn > 0) return dyn_rmax_all;   // (refusal(): no rectangle is larger)
    double r = 0.0;
    for (int j = 0; j < n_sobb; ++j) r = std::fmax(r, rects[(size_t)j * kRectRow + 6]);
    return r;
}

// Steps of the table a plan reads, relative to dyn_t0: [first, last].  The kernels ask at time_step0 + i * factor, i = 0 .. N.
inline void plan_window(int time_step0, int N, int factor, int dyn_t0, long long &first, long long &last) {
    const long long a = (long long)time_step0 - dyn_t0, b = a + (long long)N * (long long)factor;
    first = a < b ? a : b;
    last = a < b ? b : a;
}

// How many steps the folded table must have for a plan (0: the plan cannot take it -- a step before dyn_t0, or too far out), and
// how many it gets when it has to be built or regrown: at least the dynamic window, the steps asked for, what it already had, plus
// the headroom.
inline int steps_needed(int time_step0, int N, int factor, int dyn_t0) {
    long long first, last;
    plan_window(time_step0, N, factor, dyn_t0, first, last);
    if (N < 0 || first < 0 || last + 1 > kMaxSteps) return 0;
    return (int)(last + 1);
}
inline int steps_grown(int have, int need, int n_steps_dyn) {
    if (need <= have) return have;
    long long s = need;
    if (n_steps_dyn > s) s = n_steps_dyn;
    s += kHeadroom;
    return (int)(s < kMaxSteps ? s : (need > kMaxSteps ? need : kMaxSteps));
}

// The folded table, `table_doubles(n_dyn + n_sobb, steps)` doubles at `out`.  `dyn`: the dynamic table as uploaded
// ([7][n_dyn][n_steps] planes, centres, rmax), may be null when n_dyn * n_steps == 0.  Dynamic rows keep their values inside their
// own window and are NaN -- absent -- beyond it; the folded rows hold the rectangle at every step.
inline void build(double *out, int n_dyn, int n_steps, const double *dyn, int n_sobb, const double *rects, int steps) {
    const int n = n_dyn + n_sobb;
    const size_t plane = (size_t)n * (size_t)steps, src_plane = (size_t)n_dyn * (size_t)n_steps;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t total = table_doubles(n, steps);
    for (size_t i = 0; i < total; ++i) out[i] = 0.0;
    double *xy = out + xy_offset(n, steps), *rmax = out + rmax_offset(n, steps);
    for (int j = 0; j < n_dyn; ++j) {
        for (int k = 0; k < steps; ++k) {
            const size_t at = (size_t)j * steps + k;
            const bool in = k < n_steps;
            for (int q = 0; q < 7; ++q) out[q * plane + at] = in ? dyn[q * src_plane + (size_t)j * n_steps + k] : nan;
            xy[2 * at] = out[at]; xy[2 * at + 1] = out[plane + at];
        }
        rmax[j] = n_steps > 0 ? dyn[rmax_offset(n_dyn, n_steps) + j] : 0.0;
    }
    for (int j = 0; j < n_sobb; ++j) {
        const double *r = rects + (size_t)j * kRectRow;
        for (int k = 0; k < steps; ++k) {
            const size_t at = (size_t)(n_dyn + j) * steps + k;
            for (int q = 0; q < 7; ++q) out[q * plane + at] = r[q];
            xy[2 * at] = r[0]; xy[2 * at + 1] = r[1];
        }
        rmax[n_dyn + j] = r[6];
    }
}

}  // namespace rpfs
