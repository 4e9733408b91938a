/*
 * rp_ensemble.h -- C ABI of the ensemble collision checker (librp_ensemble.so): K given trajectories against M sampled
 * predictions of the dynamic obstacles ("members") in one call.
 *
 * rp_check.h answers which of K trajectories is free against ONE dynamic-obstacle table.  A caller that plans against
 * uncertain predictions has M tables -- M sampled futures of the same obstacles -- and asks, per trajectory, in how many
 * futures it collides, and which is the first trajectory that collides in at most so many of them.  With rp_check.h that is
 * M rounds of rp_checker_set_obstacles + rp_checker_check: M table uploads, M uploads of the same poses, M tests of the same
 * static shapes, M device round trips.  Here the poses are uploaded once, the static shapes are tested once per wavefront,
 * the members are spread over the grid and the answer comes back in one round trip.
 *
 * The tests are those of rp_check.h (RP_TRAJ_POSES, RP_TRAJ_SWEPT: both tests of ReactivePlanner._check_collisions) with
 * the narrow phase of the planner's kernels (csrc/rp_device.h), so a verdict per (trajectory, member) is the one
 * rp_checker_check gives on that member's table and the one a plan would have given.
 *
 * An rp_ensemble shares nothing with a planning context (rp_ctx) or a checker (rp_checker): it owns its stream, its tables
 * and its buffers.  Built from csrc/rp_ensemble.hip alone; the other two libraries are not touched by it.
 *
 * Conventions: those of rp_amd.h and rp_check.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that
 * are only read or written during the call, 0 or a negative RP_E* code as the return value, the message from
 * rp_ensemble_last_error, nothing throws across the ABI.  Calls on one object must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (rp_params.struct_size is not this
 * library's sizeof(rp_params)), RP_ESTATE (the object has no device: rp_ensemble_create had failed), RP_ENOMEM, RP_EHIP (a
 * HIP call failed; the message has its text).
 * rp_ensemble_create, rp_ensemble_set_static, rp_ensemble_set_members, rp_ensemble_check and rp_ensemble_destroy make the
 * object's device the calling thread's current HIP device (hipSetDevice) and leave it so.
 */
#ifndef RP_ENSEMBLE_H
#define RP_ENSEMBLE_H

#include "rp_amd.h" /* rp_params, RP_E* */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_ENSEMBLE_ABI_VERSION 1

typedef struct rp_ensemble rp_ensemble;

int rp_ensemble_abi_version(void);
/* *out is set even when the call fails (rp_ensemble_last_error then has the reason; destroy it all the same).
 * A fresh object has no static shapes and one member without dynamic obstacles. */
int rp_ensemble_create(rp_ensemble **out, int device);
void rp_ensemble_destroy(rp_ensemble *e);
const char *rp_ensemble_last_error(const rp_ensemble *e);

/* Most members, most dynamic rows of all members together (n_members * n_dyn * n_steps), most poses of one call
 * (K * n_poses) and most verdicts of one call (K * n_members): beyond any of them a call is refused with RP_EINVAL. */
#define RP_ENSEMBLE_MAX_MEMBERS 4096
#define RP_ENSEMBLE_MAX_DYN_ROWS ((int64_t)1 << 22)
#define RP_ENSEMBLE_MAX_POSES ((int64_t)1 << 24)
#define RP_ENSEMBLE_MAX_VERDICTS ((int64_t)1 << 24)

/* The static tables of rp_checker_set_obstacles, same meaning: sobb[n_sobb][5] = cx,cy,theta,half_l,half_w; tri[n_tri][6];
 * circ[n_circ][3] = cx,cy,r.  They do not depend on the member: a hit on one of them counts in every member.
 * Replaces the static shapes of an earlier call and leaves the members as they are.
 * RP_EINVAL: a negative count, a null table with a positive count. */
int rp_ensemble_set_static(rp_ensemble *e, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri,
                           int32_t n_circ, const double *circ);

/* dyn[n_members][n_dyn][n_steps][5]: member m's table of the dynamic rectangles, rows as in rp_checker_set_obstacles, for
 * scenario time steps dyn_t0 .. dyn_t0+n_steps-1 (cx = NaN: absent).  n_dyn == 0 or n_steps == 0, dyn may then be NULL:
 * n_members members without dynamic obstacles.  Replaces the members of an earlier call and leaves the static shapes as
 * they are.  RP_EINVAL: n_members < 1 or > RP_ENSEMBLE_MAX_MEMBERS; a negative count; n_members * n_dyn * n_steps >
 * RP_ENSEMBLE_MAX_DYN_ROWS; null dyn with rows. */
int rp_ensemble_set_members(rp_ensemble *e, int32_t n_members, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0,
                            const double *dyn);

#ifndef RP_TRAJ_POSES /* (the two mode bits of rp_check.h, same values) */
#define RP_TRAJ_POSES 1u /* per-pose test */
#define RP_TRAJ_SWEPT 2u /* continuous test */
#endif

/* mode, K, n_poses, x, y, theta, len and the fields read from params (wb_rear_axle, length, width, time_step0, factor)
 * mean what they mean in rp_checker_check:
 *   ego rectangle of pose i: centre (x, y) moved by wb_rear_axle along theta, half extents length/2, width/2.
 *   RP_TRAJ_POSES: pose i against the static shapes and against the member's dynamic obstacles at scenario time index
 *     time_step0 + i * factor.
 *   RP_TRAJ_SWEPT: segment i (i < len[k] - 1) = the tight rectangle around the ego rectangles of poses i and i + 1, against
 *     the static shapes and the member's table at time index time_step0 + i -- the factor does not enter.
 *   A time index outside the dynamic table, or a row whose cx is NaN: the obstacle is absent.
 * first_pose_hit[k][m], first_segment_hit[k][m] ([K][n_members]): smallest colliding pose / segment of trajectory k in member
 *   m, -1 if none (segments: also for len[k] < 2).
 * members_hit[k]: members in which trajectory k has any requested hit.
 * *first_free: smallest k with members_hit[k] <= max_members_hit, -1 if there is none.  *n_over: trajectories with
 *   members_hit[k] > max_members_hit.  Both are reduced on the device.
 * Every output pointer may be NULL.  RP_EINVAL: mode without a bit or with an unknown one; K < 0; n_poses < 1;
 * K * n_poses > RP_ENSEMBLE_MAX_POSES; K * n_members > RP_ENSEMBLE_MAX_VERDICTS; max_members_hit < 0 or > n_members; a len[k]
 * out of range; first_pose_hit without RP_TRAJ_POSES or first_segment_hit without RP_TRAJ_SWEPT; null poses with K > 0.
 * K == 0 succeeds with *first_free = -1, *n_over = 0.
 * With one member and max_members_hit = 0 every output equals rp_checker_check's on the same tables (members_hit[k] is 0 or
 * 1, *n_over its *n_hit). */
int rp_ensemble_check(rp_ensemble *e, const rp_params *params, uint32_t mode, int64_t K, int32_t n_poses, const double *x,
                      const double *y, const double *theta, const int32_t *len, int32_t max_members_hit,
                      int32_t *first_pose_hit, int32_t *first_segment_hit, int32_t *members_hit, int64_t *first_free,
                      int64_t *n_over);

#ifdef __cplusplus
}
#endif
#endif /* RP_ENSEMBLE_H */
