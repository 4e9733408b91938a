// rp_clearance.hip -- librp_clearance.so: the clearance query of include/rp_clearance.h (MI355X / gfx950).
//
// K given trajectories x n poses x M obstacles, as rp_check.hip, but the answer is a distance: per pose the Euclidean distance of
// the ego rectangle to the nearest obstacle present and that obstacle's id, reduced to a minimum per trajectory and to three
// scalars per call.  The boolean narrow phase is the planner's (rp_device.h: Obb, obb_obb, obb_tri, obb_circ) and runs first, so
// "clearance 0" is the checker's verdict; the distances rectangle-rectangle, rectangle-triangle and rectangle-circle are new and
// live here.  The tables are laid out as the checker's: a wavefront is 64 consecutive poses of one trajectory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_device.h"
#include "rp_obstacle_tables.h"   // the tables' layout and host builder: shared with the checkers and the picks
#include "rp_session.h"           // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_clearance.h"

namespace {

constexpr int CL_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int CL_WAVES = CL_BLOCK / 64;
constexpr int CL_ROW = OT_ROW;                  // doubles per static row (rp_obstacle_tables.h)
constexpr int CL_LDS_ROWS = 128;                // static rows staged in LDS (10 KiB per workgroup); more: read from device memory
constexpr int CL_FINAL_BLOCK = 1024;            // the one workgroup of rp_clearance_final_kernel
constexpr double CL_TINY = RP_CLEARANCE_TINY;

// The tables of rp_obstacle_tables.h; the order of the static rows and then of the dynamic obstacles is the order of the ids.  Every
// lane of a wavefront reads the same static row (a broadcast from LDS, or a scalar load); the dynamic planes are laid out so that the
// lanes of a wavefront -- consecutive time indices -- read consecutive addresses.
struct ClTables {
    const double *stat;
    const double *dyn;
    int32_t n_sobb, n_tri, n_circ, n_dyn, n_steps, dyn_t0;
};

typedef const double __attribute__((address_space(3))) *lds_cdouble;

// ---- the distances ---------------------------------------------------------------------------------------------------------
// All of them between closed convex sets that the boolean test found disjoint: the minimum is then attained at a vertex of one
// shape and the boundary of the other.  They work on squared distances; the caller takes one square root of the minimum (the square
// root is monotone, so that is the minimum of the distances).

// point to rectangle, in the rectangle's own frame (the clamp of obb_circ); 0 inside
__device__ __forceinline__ double pt_obb_d2(const Obb &r, double px, double py) {
    const double qx = px - r.cx, qy = py - r.cy;
    const double lx = qx * r.ux + qy * r.uy, ly = qy * r.ux - qx * r.uy;
    const double dx = fmax(fabs(lx) - r.hl, 0.0), dy = fmax(fabs(ly) - r.hw, 0.0);
    return dx * dx + dy * dy;
}

// point p to the segment a b (a == b: the point a)
__device__ __forceinline__ double pt_seg_d2(double px, double py, double ax, double ay, double bx, double by) {
    const double ex = bx - ax, ey = by - ay, qx = px - ax, qy = py - ay;
    const double den = ex * ex + ey * ey;
    double t = den > 0.0 ? (qx * ex + qy * ey) / den : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    const double dx = qx - t * ex, dy = qy - t * ey;
    return dx * dx + dy * dy;
}

struct Corners { double x[4], y[4]; };

__device__ __forceinline__ Corners obb_corners(const Obb &r) {
    const double lx = r.hl * r.ux, ly = r.hl * r.uy, wx = -r.hw * r.uy, wy = r.hw * r.ux;
    Corners c;
    c.x[0] = r.cx + lx + wx; c.y[0] = r.cy + ly + wy;
    c.x[1] = r.cx - lx + wx; c.y[1] = r.cy - ly + wy;
    c.x[2] = r.cx - lx - wx; c.y[2] = r.cy - ly - wy;
    c.x[3] = r.cx + lx - wx; c.y[3] = r.cy + ly - wy;
    return c;
}

// rectangle e (corners ec) to rectangle b: eight point-to-rectangle distances
__device__ __forceinline__ double obb_obb_d2(const Obb &e, const Corners &ec, const Obb &b) {
    const Corners bc = obb_corners(b);
    double m = pt_obb_d2(b, ec.x[0], ec.y[0]);
#pragma unroll
    for (int q = 1; q < 4; ++q) m = fmin(m, pt_obb_d2(b, ec.x[q], ec.y[q]));
#pragma unroll
    for (int q = 0; q < 4; ++q) m = fmin(m, pt_obb_d2(e, bc.x[q], bc.y[q]));
    return m;
}

// rectangle e to the triangle t = x1, y1 .. y3: its three vertices against the rectangle, the rectangle's four against its three edges
__device__ __forceinline__ double obb_tri_d2(const Obb &e, const Corners &ec, const double *t) {
    double m = pt_obb_d2(e, t[0], t[1]);
    m = fmin(m, pt_obb_d2(e, t[2], t[3]));
    m = fmin(m, pt_obb_d2(e, t[4], t[5]));
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int s2 = (s + 1) % 3;
#pragma unroll
        for (int q = 0; q < 4; ++q) m = fmin(m, pt_seg_d2(ec.x[q], ec.y[q], t[2 * s], t[2 * s + 1], t[2 * s2], t[2 * s2 + 1]));
    }
    return m;
}

// a computed distance of a pair the boolean test found disjoint: never 0 (and never NaN)
__device__ __forceinline__ double positive(double d) { return d > 0.0 ? d : CL_TINY; }

// The running minimum of a lane: `d` starts at the cutoff with id -1 and only ever falls.  Obstacles are offered in ascending id
// order and one replaces the minimum only when it is strictly smaller (or equal to the cutoff while nothing was found yet), so the
// id is the smallest that attains the minimum.
struct Nearest {
    double d;
    int32_t id;
    __device__ __forceinline__ void offer(double v, int32_t j) {
        if (v < d || (id < 0 && v == d)) { d = v; id = j; }
    }
};

// Branch and bound in front of every exact computation: the pair's distance is at least the distance of the centres minus both
// bounding radii, so it cannot be smaller than the running minimum m when centre distance > r + m.  The small relative margin keeps
// the bound from ever rejecting a pair whose computed distance would have been smaller or equal.  False for NaN (absent), true for
// m = +inf.  m >= 0 makes this a superset of the checker's own bounding-circle test (near_hit), which decides whether the boolean
// test runs at all -- so a hit is found exactly where the checker finds it.
__device__ __forceinline__ bool may_beat(double dist2, double rr, double m) { const double s = rr + m; return dist2 <= s * s * 1.000001; }
__device__ __forceinline__ bool near_hit(double dist2, double rr) { return dist2 <= rr * rr * 1.000001; }

// Clearance of rectangle e (radius r of a circle around it) at scenario time index t, for the lanes that `want` it.  Every lane of
// the wavefront calls this.  A lane that has reached 0 is done.
template <bool LDS>
__device__ __forceinline__ Nearest cl_nearest(const ClTables &tb, const double *lds_rows, const Obb &e, double r, long long t, bool want,
                                              double cutoff) {
    Nearest best = {cutoff, -1};
    const Corners ec = obb_corners(e);
    auto row = [&](int j, int q) -> double {
        if constexpr (LDS) return ((lds_cdouble)lds_rows)[j * CL_ROW + q];
        else return ((gcdouble)tb.stat)[(size_t)j * CL_ROW + q];
    };
    const int n_static = tb.n_sobb + tb.n_tri + tb.n_circ;
    for (int j = 0; j < n_static; ++j) {   // wave-uniform
        const double dx = row(j, 6) - e.cx, dy = row(j, 7) - e.cy, rr = r + row(j, 8);
        const double dist2 = dx * dx + dy * dy;
        if (want && best.d > 0.0 && may_beat(dist2, rr, best.d)) {
            const bool close = near_hit(dist2, rr);
            double d;
            if (j < tb.n_sobb) {
                const Obb b = {row(j, 0), row(j, 1), row(j, 2), row(j, 3), row(j, 4), row(j, 5)};
                d = close && obb_obb(e, b) ? 0.0 : positive(sqrt(obb_obb_d2(e, ec, b)));
            } else if (j < tb.n_sobb + tb.n_tri) {
                const double tv[6] = {row(j, 0), row(j, 1), row(j, 2), row(j, 3), row(j, 4), row(j, 5)};
                d = close && obb_tri(e, tv) ? 0.0 : positive(sqrt(obb_tri_d2(e, ec, tv)));
            } else {
                const double cx = row(j, 0), cy = row(j, 1), cr = row(j, 2);
                d = close && obb_circ(e, cx, cy, cr) ? 0.0 : positive(sqrt(pt_obb_d2(e, cx, cy)) - cr);
            }
            best.offer(d, j);
        }
    }
    // dynamic rectangles at the lane's own time index; outside the table: absent
    const long long k = t - (long long)tb.dyn_t0;
    const bool in_table = want && k >= 0 && k < (long long)tb.n_steps;
    const size_t kc = in_table ? (size_t)k : 0;
    const size_t plane = (size_t)tb.n_dyn * (size_t)tb.n_steps;
    const gcdouble dyn = (gcdouble)tb.dyn;
    for (int j = 0; j < tb.n_dyn; ++j) {
        const bool open = in_table && best.d > 0.0;
        if (!__any(open)) break;   // the wavefront goes on while any lane is above 0
        const gcdouble o = dyn + (size_t)j * (size_t)tb.n_steps + kc;
        const double cx = o[0], cy = o[plane], rr = r + o[6 * plane];
        const double dx = cx - e.cx, dy = cy - e.cy;
        const double dist2 = dx * dx + dy * dy;
        if (open && may_beat(dist2, rr, best.d)) {   // false for NaN: absent
            const Obb b = {cx, cy, o[2 * plane], o[3 * plane], o[4 * plane], o[5 * plane]};
            const double d = near_hit(dist2, rr) && obb_obb(e, b) ? 0.0 : positive(sqrt(obb_obb_d2(e, ec, b)));
            best.offer(d, n_static + j);
        }
    }
    return best;
}

// A lane is a pose, a wavefront 64 consecutive poses of one trajectory: wavefront w of the grid = chunk w % nchunk of trajectory
// w / nchunk.  poses: planes x | y | theta, each [K][n].  pose_clear / pose_id [K][n] receive every pose's clearance and nearest id
// (+inf and -1 above the cutoff, without an obstacle, and behind the trajectory's end).
template <bool LDS>
__global__ __launch_bounds__(CL_BLOCK) void rp_clearance_pose_kernel(ClTables tb, const double *poses, const int32_t *len, int K, int n, int nchunk,
                                                                     double wb_rear_axle, double hl, double hw, int t0, int factor, double cutoff,
                                                                     double *pose_clear, int32_t *pose_id) {
    __shared__ double sh_rows[LDS ? CL_LDS_ROWS * CL_ROW : 1];
    if (LDS) {
        const int nd = (tb.n_sobb + tb.n_tri + tb.n_circ) * CL_ROW;   // <= CL_LDS_ROWS * CL_ROW: the host picks this variant
        for (int q = threadIdx.x; q < nd; q += CL_BLOCK) sh_rows[q] = tb.stat[q];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * CL_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= (long long)K * nchunk) return;   // (a whole wavefront, behind the only barrier)
    const int k = (int)(w / nchunk), chunk = (int)(w % nchunk);
    const int i = chunk * 64 + lane;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    const bool have = i < L;
    const size_t plane = (size_t)K * (size_t)n;
    const size_t at = (size_t)k * (size_t)n + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never asked
    double s, c;
    sincos(poses[2 * plane + at], &s, &c);
    const Obb ego = {poses[at] + wb_rear_axle * c, poses[plane + at] + wb_rear_axle * s, c, s, hl, hw};
    const Nearest best = cl_nearest<LDS>(tb, sh_rows, ego, sqrt(hl * hl + hw * hw), (long long)t0 + (long long)i * factor, have, cutoff);
    if (i < n) {
        const size_t out = (size_t)k * (size_t)n + (size_t)i;
        const bool found = have && best.id >= 0;
        pose_clear[out] = found ? best.d : __builtin_huge_val();
        pose_id[out] = found ? best.id : -1;
    }
}

// One wavefront per trajectory: the minimum of its n pose clearances, the smallest pose that attains it and that pose's obstacle.
// Exact -- a minimum of doubles, ties to the smaller index -- whatever the launch shape.
__global__ __launch_bounds__(CL_BLOCK) void rp_clearance_traj_kernel(int K, int n, const double *pose_clear, const int32_t *pose_id, double *min_clear,
                                                                     int32_t *min_pose, int32_t *nearest) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    if (k >= K) return;
    const double *pc = pose_clear + (size_t)k * (size_t)n;
    double v = __builtin_huge_val();
    int at = n;   // (above every pose)
    for (int i = lane; i < n; i += 64) {   // ascending: a lane keeps the first of equal values
        const double c = pc[i];
        if (c < v || (c == v && i < at)) { v = c; at = i; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oat = __shfl_xor(at, off);
        if (ov < v || (ov == v && oat < at)) { v = ov; at = oat; }
    }
    if (lane == 0) {
        const bool finite = v < __builtin_huge_val();
        min_clear[k] = v;
        min_pose[k] = finite ? at : -1;
        nearest[k] = finite ? pose_id[(size_t)k * (size_t)n + (size_t)at] : -1;
    }
}

// The three scalars of a call, by ONE workgroup that strides over the K minima (no atomics, nothing to initialise, the same result
// whatever K): red[0] = smallest k with min_clear[k] > margin (~0: none), red[1] = trajectories with min_clear[k] <= margin,
// red[2] = the k of the largest minimum, the smallest such k.  Non-negative doubles (+inf included) order like their bit patterns.
__global__ __launch_bounds__(CL_FINAL_BLOCK) void rp_clearance_final_kernel(long long K, const double *min_clear, double margin, unsigned long long *red) {
    __shared__ unsigned long long sh_first[CL_FINAL_BLOCK / 64], sh_below[CL_FINAL_BLOCK / 64], sh_bits[CL_FINAL_BLOCK / 64], sh_best[CL_FINAL_BLOCK / 64];
    unsigned long long first = ~0ull, below = 0ull, bits = 0ull, bestk = ~0ull;
    for (long long k = threadIdx.x; k < K; k += CL_FINAL_BLOCK) {   // ascending: a thread keeps the first of equal values
        const double v = min_clear[k];
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        if (v > margin) first = first < (unsigned long long)k ? first : (unsigned long long)k;
        else ++below;
        if (bestk == ~0ull || b > bits) { bits = b; bestk = (unsigned long long)k; }
    }
    auto merge = [&](unsigned long long of, unsigned long long ob, unsigned long long obits, unsigned long long obest) {
        first = of < first ? of : first;
        below += ob;
        if (obest != ~0ull && (bestk == ~0ull || obits > bits || (obits == bits && obest < bestk))) { bits = obits; bestk = obest; }
    };
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long of = __shfl_xor(first, off), ob = __shfl_xor(below, off), obits = __shfl_xor(bits, off), obest = __shfl_xor(bestk, off);
        merge(of, ob, obits, obest);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh_first[wave] = first; sh_below[wave] = below; sh_bits[wave] = bits; sh_best[wave] = bestk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < CL_FINAL_BLOCK / 64; ++q) merge(sh_first[q], sh_below[q], sh_bits[q], sh_best[q]);
        red[0] = first; red[1] = below; red[2] = bestk;
    }
}

}  // namespace

struct rp_clearance : RpSession {
    ClTables tb = {nullptr, nullptr, 0, 0, 0, 0, 0, 0};
    RpTable d_stat, d_dyn;
};

extern "C" {

int rp_clearance_abi_version(void) { return RP_CLEARANCE_ABI_VERSION; }

int rp_clearance_create(rp_clearance **out, int device) { return session_create(out, device); }

void rp_clearance_destroy(rp_clearance *cl) { session_destroy(cl); }

const char *rp_clearance_last_error(const rp_clearance *cl) { return session_last_error(cl, "null clearance object"); }

int rp_clearance_set_obstacles(rp_clearance *cl, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ,
                               const double *circ, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn) {
    if (!cl) return RP_EINVAL;
    if (!cl->stream) return fail(cl, RP_ESTATE, "rp_clearance_set_obstacles: the object has no device (rp_clearance_create failed)");
    std::vector<double> a, e;
    std::string msg;
    int rc = ot_refuse("rp_clearance_set_obstacles", n_sobb, sobb, n_tri, tri, n_circ, circ, n_dyn, n_steps, dyn, msg);
    if (rc != RP_OK) return fail(cl, rc, msg);
    if ((int64_t)n_sobb + n_tri + n_circ + n_dyn > INT32_MAX) return fail(cl, RP_EINVAL, "rp_clearance_set_obstacles: too many obstacles for an int32 id");
    rc = ot_fill("rp_clearance_set_obstacles", n_sobb, sobb, n_tri, tri, n_circ, circ, n_dyn, n_steps, dyn, a, e, msg);
    if (rc != RP_OK) return fail(cl, rc, msg);
    if ((rc = replace_tables(cl, {{&cl->d_stat, &a}, {&cl->d_dyn, &e}})) != RP_OK) return rc;
    const bool any_dyn = !e.empty();
    cl->tb = {cl->d_stat.p, cl->d_dyn.p, n_sobb, n_tri, n_circ, any_dyn ? n_dyn : 0, any_dyn ? n_steps : 0, dyn_t0};
    return RP_OK;
}

int rp_clearance_query(rp_clearance *cl, const rp_params *p, int64_t K, int32_t n_poses, const double *x, const double *y, const double *theta,
                       const int32_t *len, double cutoff, double margin, double *pose_clearance, double *min_clearance, int32_t *min_pose,
                       int32_t *nearest, int64_t *first_clear, int64_t *n_below, int64_t *best) {
    if (!cl) return RP_EINVAL;
    if (!p) return fail(cl, RP_EINVAL, "rp_clearance_query: null params");
    if (p->struct_size != sizeof(rp_params)) return fail(cl, RP_EABI, "rp_clearance_query: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (K < 0 || n_poses < 1) return fail(cl, RP_EINVAL, "rp_clearance_query: K < 0 or n_poses < 1");
    if (K > RP_CLEARANCE_MAX_POSES || K * (int64_t)n_poses > RP_CLEARANCE_MAX_POSES)
        return fail(cl, RP_EINVAL, "rp_clearance_query: K * n_poses beyond RP_CLEARANCE_MAX_POSES");
    if (!(cutoff > 0.0)) return fail(cl, RP_EINVAL, "rp_clearance_query: cutoff must be positive (+inf allowed)");
    if (!(margin >= 0.0)) return fail(cl, RP_EINVAL, "rp_clearance_query: margin must be >= 0");
    if (K > 0 && (!x || !y || !theta)) return fail(cl, RP_EINVAL, "rp_clearance_query: null poses");
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(cl, RP_EINVAL, "rp_clearance_query: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (K == 0) {
        if (first_clear) *first_clear = -1;
        if (n_below) *n_below = 0;
        if (best) *best = -1;
        return RP_OK;
    }
    if (!cl->stream) return fail(cl, RP_ESTATE, "rp_clearance_query: the object has no device (rp_clearance_create failed)");
    RP_TRY(cl, hipSetDevice(cl->device));
    const size_t P = (size_t)K * (size_t)n_poses, Kz = (size_t)K;
    const size_t in_bytes = 3 * P * sizeof(double) + (len ? Kz * sizeof(int32_t) : 0);
    // results on the device: scalars | min_clearance [K] | min_pose [K] | nearest [K] | (8-byte aligned) pose clearance [P] | pose id [P];
    // a call copies back the front of it, as far as it asks for
    const size_t minc_off = 4 * sizeof(unsigned long long), minp_off = minc_off + Kz * sizeof(double), near_off = minp_off + Kz * sizeof(int32_t);
    const size_t pc_off = (near_off + Kz * sizeof(int32_t) + 7) & ~(size_t)7, id_off = pc_off + P * sizeof(double);
    const size_t dev_bytes = id_off + P * sizeof(int32_t);
    const size_t back_bytes = pose_clearance ? id_off : pc_off;
    const int rc = grow_call(cl, "rp_clearance_query", in_bytes, back_bytes, dev_bytes);
    if (rc != RP_OK) return rc;
    double *h_poses = static_cast<double *>(cl->h_in.p);
    std::memcpy(h_poses, x, P * sizeof(double));
    std::memcpy(h_poses + P, y, P * sizeof(double));
    std::memcpy(h_poses + 2 * P, theta, P * sizeof(double));
    if (len) std::memcpy(h_poses + 3 * P, len, Kz * sizeof(int32_t));
    RP_TRY(cl, hipMemcpyAsync(cl->d_in.p, cl->h_in.p, in_bytes, hipMemcpyHostToDevice, cl->stream));
    char *d_out = static_cast<char *>(cl->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(d_out);
    double *d_minc = reinterpret_cast<double *>(d_out + minc_off), *d_pc = reinterpret_cast<double *>(d_out + pc_off);
    int32_t *d_minp = reinterpret_cast<int32_t *>(d_out + minp_off), *d_near = reinterpret_cast<int32_t *>(d_out + near_off);
    int32_t *d_id = reinterpret_cast<int32_t *>(d_out + id_off);
    const double *d_poses = static_cast<const double *>(cl->d_in.p);
    const int32_t *d_len = len ? reinterpret_cast<const int32_t *>(d_poses + 3 * P) : nullptr;
    const int nchunk = (n_poses + 63) / 64;
    const long long waves = (long long)K * nchunk;
    const unsigned grid = (unsigned)((waves + CL_WAVES - 1) / CL_WAVES);
    const bool in_lds = cl->tb.n_sobb + cl->tb.n_tri + cl->tb.n_circ <= CL_LDS_ROWS;
    const auto kernel = in_lds ? rp_clearance_pose_kernel<true> : rp_clearance_pose_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(CL_BLOCK), 0, cl->stream, cl->tb, d_poses, d_len, (int)K, (int)n_poses, nchunk, p->wb_rear_axle,
                       0.5 * p->length, 0.5 * p->width, (int)p->time_step0, (int)p->factor, cutoff, d_pc, d_id);
    RP_TRY(cl, hipGetLastError());
    hipLaunchKernelGGL(rp_clearance_traj_kernel, dim3((unsigned)((K + CL_WAVES - 1) / CL_WAVES)), dim3(CL_BLOCK), 0, cl->stream, (int)K, (int)n_poses,
                       d_pc, d_id, d_minc, d_minp, d_near);
    RP_TRY(cl, hipGetLastError());
    hipLaunchKernelGGL(rp_clearance_final_kernel, dim3(1), dim3(CL_FINAL_BLOCK), 0, cl->stream, (long long)K, d_minc, margin, d_red);
    RP_TRY(cl, hipGetLastError());
    RP_TRY(cl, hipMemcpyAsync(cl->h_out.p, cl->d_out.p, back_bytes, hipMemcpyDeviceToHost, cl->stream));
    RP_TRY(cl, hipStreamSynchronize(cl->stream));
    const char *h_out = static_cast<const char *>(cl->h_out.p);
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    if (first_clear) *first_clear = h_red[0] < (unsigned long long)K ? (int64_t)h_red[0] : -1;
    if (n_below) *n_below = (int64_t)h_red[1];
    if (best) *best = h_red[2] < (unsigned long long)K ? (int64_t)h_red[2] : -1;
    if (min_clearance) std::memcpy(min_clearance, h_out + minc_off, Kz * sizeof(double));
    if (min_pose) std::memcpy(min_pose, h_out + minp_off, Kz * sizeof(int32_t));
    if (nearest) std::memcpy(nearest, h_out + near_off, Kz * sizeof(int32_t));
    if (pose_clearance) std::memcpy(pose_clearance, h_out + pc_off, P * sizeof(double));
    return RP_OK;
}

}  // extern "C"
