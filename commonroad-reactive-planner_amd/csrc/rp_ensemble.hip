// rp_ensemble.hip -- librp_ensemble.so: the ensemble collision checker of include/rp_ensemble.h (MI355X / gfx950).
//
// K given trajectories x n poses against M sampled predictions ("members") of the dynamic obstacles, in one call.  The narrow
// phase is the planner's (rp_device.h: Obb, obb_obb, obb_tri, obb_circ, merge_swept) behind the bounding-circle pre-test of
// rp_check.hip, so a verdict per (trajectory, member) is the boolean rp_checker_check and the planner's kernels produce.  The
// tables and their host-side packing are those of rp_obstacle_tables.h; the walk of the static rows is restated here, and the two
// libraries share no object code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rp_device.h"
#include "rp_obstacle_tables.h"   // the tables' layout and host builder: shared with the checker, the clearance query and the picks
#include "rp_session.h"           // the host session: the object's first fields, fail, RP_TRY, the blocks of a call, the upload of a table
#include "../../include/rp_ensemble.h"

namespace {

constexpr int EN_BLOCK = 256;                   // four wavefronts per workgroup
constexpr int EN_WAVES = EN_BLOCK / 64;
constexpr int EN_ROW = OT_ROW;                  // doubles per static row (rp_obstacle_tables.h)
constexpr int EN_LDS_ROWS = 128;                // static rows staged in LDS (10 KiB per workgroup); more: read from device memory
constexpr int32_t EN_NONE = 0x7f7f7f7f;         // "no hit yet" of the first-hit matrices (a byte fill), above every pose index
// Members one wavefront tests side by side (the member blocks are the grid's y dimension).  A larger block shares the rectangles
// and the static test of a wavefront among more members, a smaller one puts more wavefronts on the device: K = 64 trajectories of
// 61 poses are 64 wavefronts per member block, far fewer than the device has SIMDs.  Chosen by measurement among 1, 2, 4, 8, 16
// (profiles/probe_ensemble.py on libraries built with -DEN_MEMBER_BLOCK_PROBE=<n>; profiles/ensemble_batch.txt).
#ifdef EN_MEMBER_BLOCK_PROBE
constexpr int EN_MEMBER_BLOCK = EN_MEMBER_BLOCK_PROBE;
#else
constexpr int EN_MEMBER_BLOCK = 2;
#endif
constexpr int EN_RED_BLOCK = 1024;              // reduce kernel: sixteen wavefronts, 64 trajectories per workgroup
constexpr int EN_RED_PER_WAVE = 64 / (EN_RED_BLOCK / 64);

static_assert(EN_MEMBER_BLOCK >= 1, "a wavefront walks at least one member");

// The tables of rp_obstacle_tables.h, the dynamic planes once per member: [M][7][n_dyn][n_steps].  Every lane of a wavefront reads
// the same static row (a broadcast from LDS, or a scalar load); the dynamic planes are laid out so that the lanes of a wavefront --
// consecutive time indices -- read consecutive addresses.
struct EnTables {
    const double *stat;
    const double *dyn;
    int32_t n_sobb, n_tri, n_circ, n_members, n_dyn, n_steps, dyn_t0;
};

typedef const double __attribute__((address_space(3))) *lds_cdouble;

// Rectangle e against the static shapes for the lanes that `want` it.  Every lane of the wavefront calls this.  r: radius of a
// circle around e (bounding-circle rejection in front of every exact test; the small relative margin keeps it from rejecting a
// pair the exact test would accept).  A lane stops at its first hit.
template <bool LDS>
__device__ __forceinline__ bool en_static_hit(const EnTables &tb, const double *lds_rows, const Obb &e, double r, bool want) {
    bool hit = false;
    auto row = [&](int j, int q) -> double {
        if constexpr (LDS) return ((lds_cdouble)lds_rows)[j * EN_ROW + q];
        else return ((gcdouble)tb.stat)[(size_t)j * EN_ROW + q];
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
    return hit;
}

// Rectangle e against the dynamic rectangles of NB members side by side, at the lane's own row kc of the table, for the lanes that
// are `open`: obstacle by obstacle, the bounding circles of all NB members are loaded before the first of them is used, so the
// wavefront waits for device memory once per obstacle, not once per (obstacle, member) -- the call is bound by that wait, not by
// arithmetic.  dyn: the first member's planes; members behind `last` repeat member `last` (their flags are not read).  The
// wavefront leaves the loop when no lane is open in any member.
template <int NB>
__device__ __forceinline__ void en_members_hit(gcdouble dyn, int last, int n_dyn, size_t n_steps, size_t plane, const Obb &e, double r,
                                               size_t kc, bool open0, bool (&hit)[NB]) {
    gcdouble base[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        hit[q] = false;
        base[q] = dyn + (size_t)(q < last ? q : last) * 7 * plane + kc;
    }
    for (int j = 0; j < n_dyn; ++j) {
        bool all_hit = true;
#pragma unroll
        for (int q = 0; q < NB; ++q) all_hit = all_hit && hit[q];
        if (!__any(open0 && !all_hit)) break;
        double cx[NB], cy[NB], rr[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const gcdouble o = base[q] + (size_t)j * n_steps;
            cx[q] = o[0]; cy[q] = o[plane]; rr[q] = r + o[6 * plane];
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const double dx = cx[q] - e.cx, dy = cy[q] - e.cy;
            if (open0 && !hit[q] && dx * dx + dy * dy <= rr[q] * rr[q] * 1.000001) {   // false for NaN: absent
                const gcdouble o = base[q] + (size_t)j * n_steps;
                const Obb b = {cx[q], cy[q], o[2 * plane], o[3 * plane], o[4 * plane], o[5 * plane]};
                hit[q] = obb_obb(e, b);
            }
        }
    }
}

// One test (per-pose or swept) of a wavefront's 64 rectangles e for the members [m_begin, m_end): the static shapes once -- their
// first hit of the wavefront, a ballot, holds in every member -- then the lanes IN FRONT of that hit against the members' tables (a
// lane behind it cannot lower the first hit).  first: row k of the [K][M] first-hit matrix, base: index of lane 0.
template <bool LDS>
__device__ __forceinline__ void en_test(const EnTables &tb, const double *lds_rows, const Obb &e, long long t, bool want, int lane, int base,
                                        int m_begin, int m_end, int32_t *first) {
    const double r = sqrt(e.hl * e.hl + e.hw * e.hw);
    const unsigned long long bs = __ballot(en_static_hit<LDS>(tb, lds_rows, e, r, want));
    const int sfirst = bs != 0 ? __ffsll(bs) - 1 : 64;
    // dynamic rectangles at the lane's own time index; outside the table: absent
    const long long kt = t - (long long)tb.dyn_t0;
    const bool open0 = want && lane < sfirst && kt >= 0 && kt < (long long)tb.n_steps;
    const size_t kc = open0 ? (size_t)kt : 0;
    const size_t plane = (size_t)tb.n_dyn * (size_t)tb.n_steps;
    const gcdouble dyn = (gcdouble)tb.dyn + (size_t)m_begin * 7 * plane;
    auto record = [&](int m, bool hit) {
        const unsigned long long bd = __ballot(hit);
        const int f = bd != 0 ? __ffsll(bd) - 1 : sfirst;
        if (f < 64 && lane == 0) atomicMin(&first[m], base + f);
    };
    const int nm = m_end - m_begin;   // wave-uniform, 1 .. EN_MEMBER_BLOCK
    if (nm == 1) {                    // (M = 1, and the last block of M = q * EN_MEMBER_BLOCK + 1)
        bool hit[1];
        en_members_hit<1>(dyn, 0, tb.n_dyn, (size_t)tb.n_steps, plane, e, r, kc, open0, hit);
        record(m_begin, hit[0]);
    } else {
        bool hit[EN_MEMBER_BLOCK];
        en_members_hit<EN_MEMBER_BLOCK>(dyn, nm - 1, tb.n_dyn, (size_t)tb.n_steps, plane, e, r, kc, open0, hit);
#pragma unroll
        for (int q = 0; q < EN_MEMBER_BLOCK; ++q)
            if (q < nm) record(m_begin + q, hit[q]);
    }
}

// A lane is a pose (and the segment that starts at it), a wavefront 64 consecutive poses of one trajectory for one block of
// EN_MEMBER_BLOCK members: wavefront w of the grid's x dimension = chunk w % nchunk of trajectory w / nchunk, blockIdx.y = member
// block.  poses: planes x | y | theta, each [K][n].  first_pose / first_seg ([K][M]) hold EN_NONE on entry (a fill in front of the
// launch) and receive the smallest colliding index by one atomicMin per (wavefront, member) that has a hit.
template <bool LDS>
__global__ __launch_bounds__(EN_BLOCK) void rp_ensemble_check_kernel(EnTables tb, const double *poses, const int32_t *len, int K, int n, int nchunk,
                                                                     uint32_t mode, double wb_rear_axle, double hl, double hw, int t0, int factor,
                                                                     int32_t *first_pose, int32_t *first_seg, unsigned long long *red) {
    __shared__ double sh_rows[LDS ? EN_LDS_ROWS * EN_ROW : 1];
    if (LDS) {
        const int nd = (tb.n_sobb + tb.n_tri + tb.n_circ) * EN_ROW;   // <= EN_LDS_ROWS * EN_ROW: the host picks this variant
        for (int q = threadIdx.x; q < nd; q += EN_BLOCK) sh_rows[q] = tb.stat[q];
        __syncthreads();
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { red[0] = ~0ull; red[1] = 0ull; }   // for rp_ensemble_reduce_kernel, behind this launch
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * EN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= (long long)K * nchunk) return;   // (a whole wavefront, behind the only barrier)
    const int k = (int)(w / nchunk), chunk = (int)(w % nchunk);
    const int M = tb.n_members;
    const int m_begin = (int)blockIdx.y * EN_MEMBER_BLOCK;
    const int m_end = m_begin + EN_MEMBER_BLOCK < M ? m_begin + EN_MEMBER_BLOCK : M;
    const int i = chunk * 64 + lane;
    const int L = len ? len[k] : n;           // 1 <= L <= n, checked by the host
    const bool have = i < L;
    const size_t plane = (size_t)K * (size_t)n;
    const size_t at = (size_t)k * (size_t)n + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never asked
    double s, c;
    sincos(poses[2 * plane + at], &s, &c);
    const Obb ego = {poses[at] + wb_rear_axle * c, poses[plane + at] + wb_rear_axle * s, c, s, hl, hw};

    if (mode & RP_TRAJ_POSES)
        en_test<LDS>(tb, sh_rows, ego, (long long)t0 + (long long)i * factor, have, lane, chunk * 64, m_begin, m_end, first_pose + (size_t)k * M);
    if (mode & RP_TRAJ_SWEPT) {
        // the rectangle of pose i + 1 comes from the next lane; the wavefront's last lane loads that pose itself
        const bool seg = i + 1 < L;
        Obb nxt = {__shfl_down(ego.cx, 1), __shfl_down(ego.cy, 1), __shfl_down(ego.ux, 1), __shfl_down(ego.uy, 1), hl, hw};
        if (lane == 63 && seg) {
            double s1, c1;
            sincos(poses[2 * plane + at + 1], &s1, &c1);
            nxt.cx = poses[at + 1] + wb_rear_axle * c1; nxt.cy = poses[plane + at + 1] + wb_rear_axle * s1; nxt.ux = c1; nxt.uy = s1;
        }
        const Obb mg = merge_swept(ego, seg ? nxt : ego);
        en_test<LDS>(tb, sh_rows, mg, (long long)t0 + (long long)i, seg, lane, chunk * 64, m_begin, m_end, first_seg + (size_t)k * M);
    }
}

// A workgroup is 64 trajectories, a wavefront EN_RED_PER_WAVE of them one after the other with its lanes across the members:
// EN_NONE -> -1 in the first-hit matrices of the requested tests and members_hit[k] by ballots.  Then one lane per trajectory:
// red[0] = smallest k with members_hit[k] <= max_hit (~0: none), red[1] = trajectories above it -- a ballot, one atomic each.
__global__ __launch_bounds__(EN_RED_BLOCK) void rp_ensemble_reduce_kernel(int K, int M, uint32_t mode, int max_hit, int32_t *first_pose,
                                                                          int32_t *first_seg, int32_t *members_hit, unsigned long long *red) {
    __shared__ int32_t sh_count[64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int q = 0; q < EN_RED_PER_WAVE; ++q) {
        const int slot = wave * EN_RED_PER_WAVE + q;
        const long long k = (long long)blockIdx.x * 64 + slot;   // wave-uniform
        int count = 0;
        if (k < K) {
            for (int m0 = 0; m0 < M; m0 += 64) {
                const int m = m0 + lane;
                const bool in = m < M;
                const size_t at = (size_t)k * (size_t)M + (size_t)(in ? m : 0);
                bool hit = false;
                if (mode & RP_TRAJ_POSES) {
                    const int32_t f = first_pose[at];
                    if (in && f >= EN_NONE) first_pose[at] = -1;
                    hit = hit || f < EN_NONE;
                }
                if (mode & RP_TRAJ_SWEPT) {
                    const int32_t f = first_seg[at];
                    if (in && f >= EN_NONE) first_seg[at] = -1;
                    hit = hit || f < EN_NONE;
                }
                count += __popcll(__ballot(in && hit));
            }
        }
        if (lane == 0) sh_count[slot] = count;
    }
    __syncthreads();
    if (wave != 0) return;
    const long long k = (long long)blockIdx.x * 64 + lane;
    const bool in = k < K;
    const int count = sh_count[lane];
    if (in) members_hit[k] = count;
    const unsigned long long bf = __ballot(in && count <= max_hit), bo = __ballot(in && count > max_hit);
    if (lane == 0) {
        if (bo != 0) atomicAdd(&red[1], (unsigned long long)__popcll(bo));
        if (bf != 0) atomicMin(&red[0], (unsigned long long)(k + (__ffsll(bf) - 1)));
    }
}

}  // namespace

struct rp_ensemble : RpSession {
    EnTables tb = {nullptr, nullptr, 0, 0, 0, 1, 0, 0, 0};   // no static shapes, one member without dynamic obstacles
    RpTable d_stat, d_dyn;
};

extern "C" {

int rp_ensemble_abi_version(void) { return RP_ENSEMBLE_ABI_VERSION; }

int rp_ensemble_create(rp_ensemble **out, int device) { return session_create(out, device); }

void rp_ensemble_destroy(rp_ensemble *en) { session_destroy(en); }

const char *rp_ensemble_last_error(const rp_ensemble *en) { return session_last_error(en, "null ensemble"); }

int rp_ensemble_set_static(rp_ensemble *en, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ,
                           const double *circ) {
    if (!en) return RP_EINVAL;
    if (!en->stream) return fail(en, RP_ESTATE, "rp_ensemble_set_static: the object has no device (rp_ensemble_create failed)");
    std::vector<double> a, none;
    std::string msg;
    int rc = ot_build("rp_ensemble_set_static", n_sobb, sobb, n_tri, tri, n_circ, circ, 0, 0, nullptr, a, none, msg);
    if (rc != RP_OK) return fail(en, rc, msg);
    if ((rc = replace_tables(en, {{&en->d_stat, &a}})) != RP_OK) return rc;
    en->tb.stat = en->d_stat.p;
    en->tb.n_sobb = n_sobb; en->tb.n_tri = n_tri; en->tb.n_circ = n_circ;
    return RP_OK;
}

int rp_ensemble_set_members(rp_ensemble *en, int32_t n_members, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn) {
    if (!en) return RP_EINVAL;
    if (!en->stream) return fail(en, RP_ESTATE, "rp_ensemble_set_members: the object has no device (rp_ensemble_create failed)");
    if (n_members < 1 || n_members > RP_ENSEMBLE_MAX_MEMBERS) return fail(en, RP_EINVAL, "rp_ensemble_set_members: n_members outside 1 .. RP_ENSEMBLE_MAX_MEMBERS");
    if (n_dyn < 0 || n_steps < 0) return fail(en, RP_EINVAL, "rp_ensemble_set_members: negative count");
    const int64_t plane64 = (int64_t)n_dyn * (int64_t)n_steps;   // < 2^62
    if (plane64 > RP_ENSEMBLE_MAX_DYN_ROWS || (int64_t)n_members * plane64 > RP_ENSEMBLE_MAX_DYN_ROWS)
        return fail(en, RP_EINVAL, "rp_ensemble_set_members: n_members * n_dyn * n_steps beyond RP_ENSEMBLE_MAX_DYN_ROWS");
    if (plane64 && !dyn) return fail(en, RP_EINVAL, "rp_ensemble_set_members: null table");
    const size_t plane = (size_t)plane64;
    std::vector<double> e;   // [M][7][n_dyn * n_steps]: member by member the planes of rp_obstacle_tables.h
    try {
        e.assign((size_t)n_members * 7 * plane, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(en, RP_ENOMEM, "rp_ensemble_set_members: host memory");
    }
    for (size_t m = 0; m < (size_t)n_members; ++m) ot_dynamic_planes(e.data() + m * 7 * plane, plane, dyn + 5 * m * plane);
    const int rc = replace_tables(en, {{&en->d_dyn, &e}});
    if (rc != RP_OK) return rc;
    en->tb.dyn = en->d_dyn.p;
    en->tb.n_members = n_members; en->tb.n_dyn = plane ? n_dyn : 0; en->tb.n_steps = plane ? n_steps : 0; en->tb.dyn_t0 = dyn_t0;
    return RP_OK;
}

int rp_ensemble_check(rp_ensemble *en, const rp_params *p, uint32_t mode, int64_t K, int32_t n_poses, const double *x, const double *y,
                      const double *theta, const int32_t *len, int32_t max_members_hit, int32_t *first_pose_hit, int32_t *first_segment_hit,
                      int32_t *members_hit, int64_t *first_free, int64_t *n_over) {
    if (!en) return RP_EINVAL;
    if (!p) return fail(en, RP_EINVAL, "rp_ensemble_check: null params");
    if (p->struct_size != sizeof(rp_params)) return fail(en, RP_EABI, "rp_ensemble_check: rp_params.struct_size is not this library's sizeof(rp_params)");
    if (mode == 0 || (mode & ~(RP_TRAJ_POSES | RP_TRAJ_SWEPT)) != 0) return fail(en, RP_EINVAL, "rp_ensemble_check: mode must be RP_TRAJ_POSES, RP_TRAJ_SWEPT or both");
    if (K < 0 || n_poses < 1) return fail(en, RP_EINVAL, "rp_ensemble_check: K < 0 or n_poses < 1");
    if (K > RP_ENSEMBLE_MAX_POSES || K * (int64_t)n_poses > RP_ENSEMBLE_MAX_POSES)
        return fail(en, RP_EINVAL, "rp_ensemble_check: K * n_poses beyond RP_ENSEMBLE_MAX_POSES");
    const int M = en->tb.n_members;
    if (K * (int64_t)M > RP_ENSEMBLE_MAX_VERDICTS) return fail(en, RP_EINVAL, "rp_ensemble_check: K * n_members beyond RP_ENSEMBLE_MAX_VERDICTS");
    if (max_members_hit < 0 || max_members_hit > M) return fail(en, RP_EINVAL, "rp_ensemble_check: max_members_hit outside 0 .. n_members");
    if (!(mode & RP_TRAJ_POSES) && first_pose_hit) return fail(en, RP_EINVAL, "rp_ensemble_check: first_pose_hit without RP_TRAJ_POSES");
    if (!(mode & RP_TRAJ_SWEPT) && first_segment_hit) return fail(en, RP_EINVAL, "rp_ensemble_check: first_segment_hit without RP_TRAJ_SWEPT");
    if (K > 0 && (!x || !y || !theta)) return fail(en, RP_EINVAL, "rp_ensemble_check: null poses");
    if (len)
        for (int64_t k = 0; k < K; ++k)
            if (len[k] < 1 || len[k] > n_poses) return fail(en, RP_EINVAL, "rp_ensemble_check: len[" + std::to_string(k) + "] outside 1 .. n_poses");
    if (K == 0) {
        if (first_free) *first_free = -1;
        if (n_over) *n_over = 0;
        return RP_OK;
    }
    if (!en->stream) return fail(en, RP_ESTATE, "rp_ensemble_check: the object has no device (rp_ensemble_create failed)");
    RP_TRY(en, hipSetDevice(en->device));
    const size_t P = (size_t)K * (size_t)n_poses, V = (size_t)K * (size_t)M;
    const size_t in_bytes = 3 * P * sizeof(double) + (len ? (size_t)K * sizeof(int32_t) : 0);
    // device results: red[2] | members_hit [K] | (16-byte boundary) first_pose [K][M] | first_seg [K][M]
    const size_t count_off = 2 * sizeof(unsigned long long);
    const size_t head_bytes = (count_off + (size_t)K * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t mat_bytes = V * sizeof(int32_t);
    // host results: the head, then the matrices the caller asked for
    const size_t h_pose_off = head_bytes, h_seg_off = head_bytes + (first_pose_hit ? mat_bytes : 0);
    const size_t h_out_bytes = h_seg_off + (first_segment_hit ? mat_bytes : 0);
    const int rc = grow_call(en, "rp_ensemble_check", in_bytes, h_out_bytes, head_bytes + 2 * mat_bytes);
    if (rc != RP_OK) return rc;
    double *h_poses = static_cast<double *>(en->h_in.p);
    std::memcpy(h_poses, x, P * sizeof(double));
    std::memcpy(h_poses + P, y, P * sizeof(double));
    std::memcpy(h_poses + 2 * P, theta, P * sizeof(double));
    if (len) std::memcpy(h_poses + 3 * P, len, (size_t)K * sizeof(int32_t));
    RP_TRY(en, hipMemcpyAsync(en->d_in.p, en->h_in.p, in_bytes, hipMemcpyHostToDevice, en->stream));
    char *d_out = static_cast<char *>(en->d_out.p);
    unsigned long long *d_red = reinterpret_cast<unsigned long long *>(d_out);
    int32_t *d_count = reinterpret_cast<int32_t *>(d_out + count_off);
    int32_t *d_first_pose = reinterpret_cast<int32_t *>(d_out + head_bytes), *d_first_seg = d_first_pose + V;
    if (mode == (RP_TRAJ_POSES | RP_TRAJ_SWEPT)) RP_TRY(en, hipMemsetAsync(d_first_pose, 0x7f, 2 * mat_bytes, en->stream));
    else RP_TRY(en, hipMemsetAsync((mode & RP_TRAJ_POSES) ? d_first_pose : d_first_seg, 0x7f, mat_bytes, en->stream));
    const double *d_poses = static_cast<const double *>(en->d_in.p);
    const int32_t *d_len = len ? reinterpret_cast<const int32_t *>(d_poses + 3 * P) : nullptr;
    const int nchunk = (n_poses + 63) / 64;
    const long long waves = (long long)K * nchunk;   // <= 2^24: the grid's x fits
    const dim3 grid((unsigned)((waves + EN_WAVES - 1) / EN_WAVES), (unsigned)((M + EN_MEMBER_BLOCK - 1) / EN_MEMBER_BLOCK));
    const bool in_lds = en->tb.n_sobb + en->tb.n_tri + en->tb.n_circ <= EN_LDS_ROWS;
    const auto kernel = in_lds ? rp_ensemble_check_kernel<true> : rp_ensemble_check_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(EN_BLOCK), 0, en->stream, en->tb, d_poses, d_len, (int)K, (int)n_poses, nchunk, mode, p->wb_rear_axle,
                       0.5 * p->length, 0.5 * p->width, (int)p->time_step0, (int)p->factor, d_first_pose, d_first_seg, d_red);
    RP_TRY(en, hipGetLastError());
    hipLaunchKernelGGL(rp_ensemble_reduce_kernel, dim3((unsigned)((K + 63) / 64)), dim3(EN_RED_BLOCK), 0, en->stream, (int)K, M, mode,
                       (int)max_members_hit, d_first_pose, d_first_seg, d_count, d_red);
    RP_TRY(en, hipGetLastError());
    char *h_out = static_cast<char *>(en->h_out.p);
    RP_TRY(en, hipMemcpyAsync(h_out, d_out, count_off + (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, en->stream));
    if (first_pose_hit) RP_TRY(en, hipMemcpyAsync(h_out + h_pose_off, d_first_pose, mat_bytes, hipMemcpyDeviceToHost, en->stream));
    if (first_segment_hit) RP_TRY(en, hipMemcpyAsync(h_out + h_seg_off, d_first_seg, mat_bytes, hipMemcpyDeviceToHost, en->stream));
    RP_TRY(en, hipStreamSynchronize(en->stream));
    const unsigned long long *h_red = reinterpret_cast<const unsigned long long *>(h_out);
    if (first_free) *first_free = h_red[0] < (unsigned long long)K ? (int64_t)h_red[0] : -1;
    if (n_over) *n_over = (int64_t)h_red[1];
    if (members_hit) std::memcpy(members_hit, h_out + count_off, (size_t)K * sizeof(int32_t));
    if (first_pose_hit) std::memcpy(first_pose_hit, h_out + h_pose_off, mat_bytes);
    if (first_segment_hit) std::memcpy(first_segment_hit, h_out + h_seg_off, mat_bytes);
    return RP_OK;
}

}  // extern "C"
