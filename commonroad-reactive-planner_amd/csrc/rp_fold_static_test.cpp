// C entry points over rp_fold_static.h for tests/test_fold_static_table.py: a host library of its own (plain C++, no device code),
// nothing of it enters librp_amd.so.
#include "rp_fold_static.h"

extern "C" {

int rpfs_test_refusal(int n_sobb, const double *rects, int n_tri, int n_circ, int n_dyn, double dyn_rmax_all, int max_rects) {
    return rpfs::refusal(n_sobb, rects, n_tri, n_circ, n_dyn, dyn_rmax_all, max_rects);
}
double rpfs_test_folded_rmax_all(int n_sobb, const double *rects, int n_dyn, double dyn_rmax_all) {
    return rpfs::folded_rmax_all(n_sobb, rects, n_dyn, dyn_rmax_all);
}
int rpfs_test_steps_needed(int time_step0, int N, int factor, int dyn_t0) { return rpfs::steps_needed(time_step0, N, factor, dyn_t0); }
int rpfs_test_steps_grown(int have, int need, int n_steps_dyn) { return rpfs::steps_grown(have, need, n_steps_dyn); }
long long rpfs_test_table_doubles(int n, int steps) { return (long long)rpfs::table_doubles(n, steps); }
long long rpfs_test_xy_offset(int n, int steps) { return (long long)rpfs::xy_offset(n, steps); }
long long rpfs_test_rmax_offset(int n, int steps) { return (long long)rpfs::rmax_offset(n, steps); }
void rpfs_test_build(double *out, int n_dyn, int n_steps, const double *dyn, int n_sobb, const double *rects, int steps) {
    rpfs::build(out, n_dyn, n_steps, dyn, n_sobb, rects, steps);
}
int rpfs_test_constant(int which) {
    return which == 0 ? rpfs::kMaxObstacles : which == 1 ? rpfs::kMaxSteps : which == 2 ? rpfs::kHeadroom : rpfs::kRectRow;
}

}  // extern "C"
