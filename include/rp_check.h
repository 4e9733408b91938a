/*
 * rp_check.h -- C ABI of the batch collision checker for trajectories the caller brings (librp_check.so).
 *
 * rp_amd.h answers one collision question on the device: which candidate of the planner's own sampling grid is free
 * (and, with rp_check_swept, whether ONE given trajectory is).  This library answers it for K given trajectories in
 * one call: the K cheapest candidates of a level, motion-primitive sets, fail-safe manoeuvres, prediction ensembles.
 * Both tests of ReactivePlanner._check_collisions, per trajectory:
 *
 *   RP_TRAJ_POSES   the per-pose test         commonroad_rp/reactive_planner.py:1033-1046
 *   RP_TRAJ_SWEPT   the continuous test       commonroad_rp/reactive_planner.py:1049-1058
 *
 * with the narrow phase of the planner's kernels (csrc/rp_device.h), so a verdict is the one a plan would have given.
 *
 * A checker shares nothing with a planning context (rp_ctx): it owns its stream, its obstacle tables and its pose and
 * result buffers, and both kinds of object can live side by side in a process.  Built from csrc/rp_check.hip alone; the
 * planning library is not touched by it.
 *
 * Conventions: those of rp_amd.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that are only read
 * or written during the call, 0 or a negative RP_E* code as the return value, the message from rp_checker_last_error,
 * nothing throws across the ABI.  Calls on one checker must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (rp_params.struct_size is not this library's
 * sizeof(rp_params)), RP_ESTATE (the checker has no device: rp_checker_create had failed), RP_ENOMEM, RP_EHIP (a HIP call failed;
 * the message has its text).
 * rp_checker_create, rp_checker_set_obstacles, rp_checker_check and rp_checker_destroy make the checker's device the calling
 * thread's current HIP device (hipSetDevice) and leave it so, as the calls on an rp_ctx do: a caller that works on another device
 * in the same thread selects it again afterwards.
 */
#ifndef RP_CHECK_H
#define RP_CHECK_H

#include "rp_amd.h" /* rp_params, RP_E* */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_CHECKER_ABI_VERSION 1

typedef struct rp_checker rp_checker;

int rp_checker_abi_version(void);
/* *out is set even when the call fails (rp_checker_last_error then has the reason; destroy it all the same). */
int rp_checker_create(rp_checker **out, int device);
void rp_checker_destroy(rp_checker *ck);
const char *rp_checker_last_error(const rp_checker *ck);

/* The flat tables of rp_set_obstacles, same meaning: sobb[n_sobb][5] = cx,cy,theta,half_l,half_w; tri[n_tri][6];
 * circ[n_circ][3] = cx,cy,r; dyn[n_dyn][n_steps][5] for scenario time steps dyn_t0 .. dyn_t0+n_steps-1 (cx = NaN: absent).
 * Replaces the tables of an earlier call.  A checker that was never given tables checks against empty ones. */
int rp_checker_set_obstacles(rp_checker *ck, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri,
                             int32_t n_circ, const double *circ, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0,
                             const double *dyn);

#define RP_TRAJ_POSES 1u /* per-pose test */
#define RP_TRAJ_SWEPT 2u /* continuous test */

/* Most poses of one call: K * n_poses beyond it is refused with RP_EINVAL. */
#define RP_CHECKER_MAX_POSES ((int64_t)1 << 24)

/* K trajectories of up to n_poses rear-axle poses each: x, y, theta are [K][n_poses]; len[k] (1 <= len[k] <= n_poses) is
 * the number of valid poses of trajectory k, len == NULL: n_poses for all.  Of params the call reads wb_rear_axle, length,
 * width, time_step0 and factor.
 *   ego rectangle of pose i: centre (x, y) moved by wb_rear_axle along theta, half extents length/2, width/2.
 *   RP_TRAJ_POSES: pose i against the static shapes and against the dynamic obstacles at scenario time index
 *     time_step0 + i * factor.  first_pose_hit[k]: smallest colliding i, -1 if none.  pose_hit[k][i]: 0 / 1, 0 for i >= len[k].
 *   RP_TRAJ_SWEPT: segment i (i < len[k] - 1) = the tight rectangle around the ego rectangles of poses i and i + 1 (as
 *     rp_check_swept), against the tables at time index time_step0 + i -- the factor does not enter.
 *     first_segment_hit[k]: smallest colliding segment, -1 if none (also for len[k] < 2).
 *   A time index outside the dynamic table, or a row whose cx is NaN: the obstacle is absent.
 *   *first_free: smallest k for which no requested test found anything, -1 if there is none (trajectories passed in cost
 *     order: the answer of the sorted walk of _check_collisions).  *n_hit: trajectories with any requested hit.  Both are
 *     reduced on the device.
 * Every output pointer may be NULL.  RP_EINVAL: mode without a bit or with an unknown one; K < 0; n_poses < 1;
 * K * n_poses > RP_CHECKER_MAX_POSES; a len[k] out of range; first_pose_hit / pose_hit without RP_TRAJ_POSES or
 * first_segment_hit without RP_TRAJ_SWEPT; null poses with K > 0.  K == 0 succeeds with *first_free = -1, *n_hit = 0. */
int rp_checker_check(rp_checker *ck, const rp_params *params, uint32_t mode, int64_t K, int32_t n_poses, const double *x,
                     const double *y, const double *theta, const int32_t *len, int32_t *first_pose_hit,
                     int32_t *first_segment_hit, uint8_t *pose_hit, int64_t *first_free, int64_t *n_hit);

#ifdef __cplusplus
}
#endif
#endif /* RP_CHECK_H */
