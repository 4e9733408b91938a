// rp_obstacle_tables.h -- the host builder of the obstacle tables the trajectory libraries upload, stated once: the static rows
// and the dynamic planes that rp_check_rules.h, rp_clearance.hip and rp_ensemble.hip walk, and the refusals in front of them.  Host
// code only; everything here has internal linkage, nothing of it is exported.
//
// Static shapes as ONE table, rectangles first, then triangles, then circles.  Row of OT_ROW doubles: [0..5] the shape -- rectangle
// cx, cy, ux, uy, hl, hw | triangle x1 .. y3 | circle cx, cy, r -- then [6..8] its bounding circle cx, cy, r and one double of padding.
// Dynamic rectangles: struct-of-arrays planes [7][n_dyn][n_steps] cx, cy, ux, uy, hl, hw, r_bound (cx = NaN: absent); an ensemble
// holds one such set of planes per member, one behind the other.
#ifndef RP_OBSTACLE_TABLES_H
#define RP_OBSTACLE_TABLES_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/rp_amd.h"

namespace {

constexpr int OT_ROW = 10;   // doubles per static row

// RP_OK, or RP_EINVAL and the message behind `who: `
inline int ot_refuse(const char *who, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ,
                     int32_t n_dyn, int32_t n_steps, const double *dyn, std::string &msg) {
    if (n_sobb < 0 || n_tri < 0 || n_circ < 0 || n_dyn < 0 || n_steps < 0 || (n_sobb && !sobb) || (n_tri && !tri) || (n_circ && !circ) ||
        (n_dyn && n_steps && !dyn)) {
        msg = std::string(who) + ": negative count or null table";
        return RP_EINVAL;
    }
    if ((int64_t)n_sobb + n_tri + n_circ > INT32_MAX / OT_ROW) {
        msg = std::string(who) + ": too many static shapes";
        return RP_EINVAL;
    }
    return RP_OK;
}

// the n_sobb + n_tri + n_circ rows at r (zeroed by the caller)
inline void ot_static_rows(double *r, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ) {
    for (int j = 0; j < n_sobb; ++j, r += OT_ROW) {   // (ux, uy from the host's cos / sin, as rp_set_obstacles)
        const double *o = sobb + 5 * (size_t)j;
        r[0] = o[0]; r[1] = o[1]; r[2] = std::cos(o[2]); r[3] = std::sin(o[2]); r[4] = o[3]; r[5] = o[4];
        r[6] = o[0]; r[7] = o[1]; r[8] = std::sqrt(o[3] * o[3] + o[4] * o[4]);
    }
    for (int j = 0; j < n_tri; ++j, r += OT_ROW) {
        const double *o = tri + 6 * (size_t)j;
        for (int q = 0; q < 6; ++q) r[q] = o[q];
        const double bx = (o[0] + o[2] + o[4]) / 3.0, by = (o[1] + o[3] + o[5]) / 3.0;
        double rr = 0.0;
        for (int q = 0; q < 3; ++q) rr = std::fmax(rr, std::hypot(o[2 * q] - bx, o[2 * q + 1] - by));
        r[6] = bx; r[7] = by; r[8] = rr;
    }
    for (int j = 0; j < n_circ; ++j, r += OT_ROW) {
        const double *o = circ + 3 * (size_t)j;
        r[0] = o[0]; r[1] = o[1]; r[2] = o[2];
        r[6] = o[0]; r[7] = o[1]; r[8] = o[2];
    }
}

// the seven planes of plane = n_dyn * n_steps rectangles at e, from the rows cx, cy, theta, hl, hw at dyn
inline void ot_dynamic_planes(double *e, size_t plane, const double *dyn) {
    for (size_t at = 0; at < plane; ++at) {
        const double *o = dyn + 5 * at;
        e[at] = o[0]; e[plane + at] = o[1];
        e[2 * plane + at] = std::cos(o[2]); e[3 * plane + at] = std::sin(o[2]);
        e[4 * plane + at] = o[3]; e[5 * plane + at] = o[4];
        e[6 * plane + at] = std::sqrt(o[3] * o[3] + o[4] * o[4]);
    }
}

// the static rows `a` and the dynamic planes `e` of counts ot_refuse has passed: RP_OK, or RP_ENOMEM and the message
inline int ot_fill(const char *who, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ,
                   int32_t n_dyn, int32_t n_steps, const double *dyn, std::vector<double> &a, std::vector<double> &e, std::string &msg) {
    const size_t plane = (size_t)n_dyn * (size_t)n_steps;
    try {
        a.assign(((size_t)n_sobb + (size_t)n_tri + (size_t)n_circ) * OT_ROW, 0.0);
        e.assign((size_t)7 * plane, 0.0);
    } catch (const std::bad_alloc &) {
        msg = std::string(who) + ": host memory";
        return RP_ENOMEM;
    }
    ot_static_rows(a.data(), n_sobb, sobb, n_tri, tri, n_circ, circ);
    ot_dynamic_planes(e.data(), plane, dyn);
    return RP_OK;
}

// a set_obstacles call's refusals and its two tables: RP_OK, or the code (RP_EINVAL, RP_ENOMEM) and the message behind `who: `
inline int ot_build(const char *who, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ, const double *circ,
                    int32_t n_dyn, int32_t n_steps, const double *dyn, std::vector<double> &a, std::vector<double> &e, std::string &msg) {
    const int rc = ot_refuse(who, n_sobb, sobb, n_tri, tri, n_circ, circ, n_dyn, n_steps, dyn, msg);
    return rc != RP_OK ? rc : ot_fill(who, n_sobb, sobb, n_tri, tri, n_circ, circ, n_dyn, n_steps, dyn, a, e, msg);
}

}  // namespace

#endif  // RP_OBSTACLE_TABLES_H
