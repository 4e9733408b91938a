// The reference-table window of the single-launch variant of rp_eval_kernel, and the bucket table it indexes.
//
// The single-launch prologue (rp_kernels.h, LON_FUSED) stages the reference-path tables in LDS: nine rows of n doubles and an int32
// bucket table for the O(1) segment lookup (rp_device.h: upper_bound_bucket).  One replanning cycle moves over a few dozen metres of
// a route of hundreds, so the host names the part a plan can touch -- vertices [win_k0, win_k0 + win_n) of every row and bucket
// entries [win_b0, win_b0 + win_nb) -- and the prologue copies only that, each entry to the place it has in the whole block.  An item
// (pair, step) reads the staged entries only if its s lies in [win_s_lo, win_s_hi); a workgroup with any other item copies the whole
// block and computes every item again.
//
// This header holds the construction of the bucket table (rp_set_reference) and the window rule (rp_plan).  Plain C++: no HIP, so
// that tests/test_table_window_host.py compiles it into a host library on a box without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace rptw {

constexpr int kLonStopping = 1;      // RP_LON_STOPPING of rp_amd.h (rp_host.hip asserts that they agree)
constexpr int kMinVertices = 96;     // shorter references are staged whole
constexpr int kMaxWindow = 128;      // the kernel holds at most 5 pieces of the window per lane
constexpr double kMaxBuckets = 8192.0;

// -- the bucket table -------------------------------------------------------------------------------------------------------------
// bucket[b] = first index with pos > pos[0] + b * hmin, hmin = the shortest segment: at most one vertex lies inside a bucket.
inline double shortest_segment(const double *pos, int n) {
    double hmin = pos[1] - pos[0];
    for (int i = 0; i + 1 < n; ++i) hmin = std::min(hmin, pos[i + 1] - pos[i]);
    return hmin;
}
// entries of the table; 0: too fine, the kernels fall back to the binary search
inline int bucket_count(const double *pos, int n, double hmin) {
    const double span = pos[n - 1] - pos[0];
    const double nbf = std::floor(span / hmin) + 1.0;
    return (nbf >= 1.0 && nbf <= kMaxBuckets) ? (int)nbf : 0;
}
inline void bucket_fill(const double *pos, int n, double hmin, int nb, int32_t *bk) {
    for (int b = 0; b < nb; ++b)
        bk[b] = (int32_t)(std::upper_bound(pos, pos + n, pos[0] + b * hmin) - pos);
}

// -- the window -------------------------------------------------------------------------------------------------------------------
struct Window {
    int32_t k0 = 0, n = 0, shift = 0, b0 = 0, nb = 0;   // n == 0: the whole block
    double s_lo = 0.0, s_hi = 0.0;
};

// Part of the reference-table block a grid plan can touch (single-launch variant: every workgroup stages the block in
// LDS -- 28 KB x 465 workgroups on cfg2 -- although one replanning cycle moves over a few dozen metres of a route of
// hundreds).  s of every valid step lies between the bounds the Hermite form of the longitudinal polynomial gives:
//   velocity keeping (quartic, v cubic from (v0, a0) to (vd, 0)):  v in [min(v0, vd) - c T |a0|, max(v0, vd) + c T |a0|], c = 4/27
//   stopping (quintic to (sf, 0, 0)):  s in [min(s0, sf), max(s0, sf)] -+ (0.2 |v0| T + 0.0173 |a0| T^2)
// An estimate, not a guarantee the kernel relies on: the kernel checks every item against [win_s_lo, win_s_hi) and stages
// the whole block when one falls outside (steps beyond the end of the route, NaN samples, ...).
inline Window table_window(const double *pos, int n, int n_buckets, double bucket_inv_h, int lon_mode, const double *x0_lon,
                           const double *T, int nT, const double *L, int nL) {
    Window w;   // whole block
    if (n < kMinVertices || n_buckets <= 0 || nT <= 0 || nL <= 0) return w;
    double Tmax = T[0], Lmin = L[0], Lmax = L[0];
    for (int i = 1; i < nT; ++i) Tmax = std::max(Tmax, T[i]);
    for (int i = 1; i < nL; ++i) { Lmin = std::min(Lmin, L[i]); Lmax = std::max(Lmax, L[i]); }
    const double s0 = x0_lon[0], v0 = x0_lon[1], a0 = std::fabs(x0_lon[2]);
    double lo, hi;
    if (lon_mode == kLonStopping) {
        const double over = 0.2 * std::fabs(v0) * Tmax + 0.0173 * a0 * Tmax * Tmax;
        lo = std::min(s0, Lmin) - over; hi = std::max(s0, Lmax) + over;
    } else {
        const double dv = (4.0 / 27.0) * Tmax * a0;
        lo = s0 + std::min(0.0, (std::min(v0, Lmin) - dv) * Tmax); hi = s0 + std::max(0.0, (std::max(v0, Lmax) + dv) * Tmax);
    }
    if (!(lo <= hi) || !(hi - lo < 1e300)) return w;   // NaN / inf samples
    const int seg_lo = (int)(std::upper_bound(pos, pos + n, lo) - pos) - 1, seg_hi = (int)(std::upper_bound(pos, pos + n, hi) - pos) - 1;
    // an item in segment seg reads vertices seg - 2 .. seg + 3 (bucket fix-ups, both interpolation pairs)
    int w0 = std::max(0, seg_lo - 3), w1 = std::min(n, seg_hi + 5);
    int shift = 4;
    while ((1 << shift) < w1 - w0) ++shift;
    const int wn = 1 << shift;
    if (wn * 2 > n || wn > kMaxWindow) return w;     // not worth a window | the kernel holds at most 5 pieces per lane
    if (w0 + wn > n) w0 = n - wn;
    w.k0 = w0; w.n = wn; w.shift = shift;
    w.s_lo = w0 == 0 ? pos[0] : pos[w0 + 2];
    w.s_hi = w0 + wn == n ? pos[n - 1] : pos[w0 + wn - 4];
    // bucket entries of [win_s_lo, win_s_hi): the kernel's index is (int)((s - pos[0]) * bucket_inv_h), clamped to n_buckets - 1
    const int b0 = std::max(0, (int)((w.s_lo - pos[0]) * bucket_inv_h) - 1);
    const int b1 = std::min(n_buckets - 1, (int)((w.s_hi - pos[0]) * bucket_inv_h) + 1);
    w.b0 = b0; w.nb = b1 - b0 + 1;
    return w;
}

}  // namespace rptw
