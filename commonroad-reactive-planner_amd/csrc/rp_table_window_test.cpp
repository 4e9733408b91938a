// C entry points over rp_table_window.h for tests/test_table_window_host.py: a host library of its own (plain C++, no device code),
// nothing of it enters librp_amd.so.
#include "rp_table_window.h"

extern "C" {

// the bucket table of a reference: returns its entries (0: none, the kernels search), *inv_h = 1 / the shortest segment; bucket
// (capacity cap entries) may be null to ask for the size alone
int rptw_test_buckets(const double *pos, int n, int32_t *bucket, int cap, double *inv_h) {
    const double hmin = rptw::shortest_segment(pos, n);
    const int nb = rptw::bucket_count(pos, n, hmin);
    if (inv_h) *inv_h = 1.0 / hmin;
    if (bucket && nb <= cap) rptw::bucket_fill(pos, n, hmin, nb, bucket);
    return nb;
}

// the window of a plan: win_i = {win_k0, win_n, win_shift, win_b0, win_nb}, win_s = {win_s_lo, win_s_hi}; returns win_n
int rptw_test_window(const double *pos, int n, int n_buckets, double bucket_inv_h, int lon_mode, const double *x0_lon, const double *T, int nT,
                     const double *L, int nL, int32_t *win_i, double *win_s) {
    const rptw::Window w = rptw::table_window(pos, n, n_buckets, bucket_inv_h, lon_mode, x0_lon, T, nT, L, nL);
    win_i[0] = w.k0; win_i[1] = w.n; win_i[2] = w.shift; win_i[3] = w.b0; win_i[4] = w.nb;
    win_s[0] = w.s_lo; win_s[1] = w.s_hi;
    return w.n;
}

int rptw_test_constant(int which) { return which == 0 ? rptw::kMinVertices : which == 1 ? rptw::kMaxWindow : (int)rptw::kMaxBuckets; }

}  // extern "C"
