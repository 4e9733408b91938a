/*
 * rp_clearance.h -- C ABI of the clearance query for trajectories the caller brings (librp_clearance.so).
 *
 * rp_check.h and rp_ensemble.h answer a yes/no question: does a pose collide?  This library answers how CLOSE the poses of K
 * given trajectories come to the obstacles: the Euclidean distance of the ego rectangle to the nearest obstacle present at the
 * pose's time index, per pose and reduced per trajectory, with the obstacle that attains it -- an obstacle-distance term of a
 * plug-in cost function, a safety margin ("the cheapest candidate that keeps 0.5 m"), a clearance profile of the chosen
 * trajectory -- in one device round trip.
 *
 * A clearance object shares nothing with a planning context (rp_ctx), a checker (rp_checker) or an ensemble checker
 * (rp_ensemble): it owns its stream, its obstacle tables and its pose and result buffers, and all of them can live side by side in
 * a process.  Built from csrc/rp_clearance.hip alone; the other libraries are not touched by it.
 *
 * Conventions: those of rp_check.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that are only read or
 * written during the call, 0 or a negative RP_E* code as the return value, the message from rp_clearance_last_error, nothing
 * throws across the ABI.  Calls on one object must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (rp_params.struct_size is not this library's
 * sizeof(rp_params)), RP_ESTATE (the object has no device: rp_clearance_create had failed), RP_ENOMEM, RP_EHIP (a HIP call failed;
 * the message has its text).
 * rp_clearance_create, rp_clearance_set_obstacles, rp_clearance_query and rp_clearance_destroy make the object's device the
 * calling thread's current HIP device (hipSetDevice) and leave it so, as the calls on an rp_checker do.
 */
#ifndef RP_CLEARANCE_H
#define RP_CLEARANCE_H

#include "rp_amd.h" /* rp_params, RP_E* */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_CLEARANCE_ABI_VERSION 1

typedef struct rp_clearance rp_clearance;

int rp_clearance_abi_version(void);
/* *out is set even when the call fails (rp_clearance_last_error then has the reason; destroy it all the same). */
int rp_clearance_create(rp_clearance **out, int device);
void rp_clearance_destroy(rp_clearance *cl);
const char *rp_clearance_last_error(const rp_clearance *cl);

/* The flat tables of rp_checker_set_obstacles, same meaning: sobb[n_sobb][5] = cx,cy,theta,half_l,half_w; tri[n_tri][6];
 * circ[n_circ][3] = cx,cy,r; dyn[n_dyn][n_steps][5] for scenario time steps dyn_t0 .. dyn_t0+n_steps-1 (cx = NaN: absent).
 * Replaces the tables of an earlier call.  An object that was never given tables queries against empty ones.
 * Obstacle ids, as rp_clearance_query reports them, follow one concatenated order: static rectangles, then triangles, then
 * circles, then dynamic obstacles -- dynamic obstacle j has the id n_sobb + n_tri + n_circ + j. */
int rp_clearance_set_obstacles(rp_clearance *cl, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri,
                               int32_t n_circ, const double *circ, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0,
                               const double *dyn);

/* Most poses of one call: K * n_poses beyond it is refused with RP_EINVAL. */
#define RP_CLEARANCE_MAX_POSES ((int64_t)1 << 24)

/* What a pair that does not collide reports when its computed distance is not positive (rounding): the smallest positive normal
 * double.  A clearance is 0.0 exactly where the planner's boolean test reports a hit, and > 0 everywhere else. */
#define RP_CLEARANCE_TINY 2.2250738585072014e-308

/* K trajectories of up to n_poses rear-axle poses each: x, y, theta are [K][n_poses]; len[k] (1 <= len[k] <= n_poses) is
 * the number of valid poses of trajectory k, len == NULL: n_poses for all.  Of params the call reads wb_rear_axle, length,
 * width, time_step0 and factor.
 *   ego rectangle of pose i: centre (x, y) moved by wb_rear_axle along theta, half extents length/2, width/2 (the checker's).
 *   Pose i meets the static shapes, and the dynamic obstacles at scenario time index time_step0 + i * factor; a time index
 *     outside the dynamic table, or a row whose cx is NaN: the obstacle is absent.
 *   Clearance of a pose: the minimum, over the obstacles present, of the Euclidean distance between the two closed sets.
 *     Exactly 0.0 where the boolean test of rp_checker_check(RP_TRAJ_POSES) reports a hit (that test runs first, bit for bit);
 *     otherwise the computed distance if it is positive, else RP_CLEARANCE_TINY -- so "clearance > 0" means "no hit" without
 *     exception.  A clearance above cutoff is reported as +inf with nearest id -1; so is a pose with no obstacle present, and
 *     every pose i >= len[k].  cutoff > 0, +inf allowed.  Values <= cutoff do not depend on cutoff.
 *   pose_clearance[K][n_poses]: the per-pose values.
 *   min_clearance[k]: the minimum over the poses; min_pose[k]: the smallest i that attains it, -1 when it is +inf;
 *     nearest[k]: the smallest obstacle id that attains the minimum at that pose, -1 when it is +inf.
 *   *first_clear: the smallest k with min_clearance[k] > margin, -1 if there is none; *n_below: the number of trajectories with
 *     min_clearance[k] <= margin; *best: the k with the largest min_clearance, the smallest such k on ties.  margin >= 0.  All
 *     three are reduced on the device.  With margin = 0 the first two are *first_free and *n_hit of
 *     rp_checker_check(RP_TRAJ_POSES) on the same tables.
 * Every output pointer may be NULL.  RP_EINVAL: K < 0; n_poses < 1; K * n_poses > RP_CLEARANCE_MAX_POSES; a len[k] out of
 * range; null poses with K > 0; cutoff <= 0 or NaN; margin < 0 or NaN.  K == 0 succeeds with *first_clear = -1, *n_below = 0,
 * *best = -1. */
int rp_clearance_query(rp_clearance *cl, const rp_params *params, int64_t K, int32_t n_poses, const double *x, const double *y,
                       const double *theta, const int32_t *len, double cutoff, double margin, double *pose_clearance,
                       double *min_clearance, int32_t *min_pose, int32_t *nearest, int64_t *first_clear, int64_t *n_below,
                       int64_t *best);

#ifdef __cplusplus
}
#endif
#endif /* RP_CLEARANCE_H */
