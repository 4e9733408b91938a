/*
 * rp_lift.h -- C ABI of the lift of curvilinear trajectories the caller brings (librp_lift.so).
 *
 * rp_score.h maps K GIVEN Cartesian trajectories into the curvilinear frame of a reference path.  This library is the opposite
 * direction: K given trajectories s, s', s'', d, d', d'' along a reference path -- a lateral QP's or MPC's output, a corridor
 * optimiser's, a learned Frenet proposal, last cycle's winner re-timed; no polynomial pair is assumed -- become x, y, theta, v, a,
 * kappa, kappa_dot and theta_cl with the reference planner's kinematic verdict (ReactivePlanner._check_kinematics in draw mode), in
 * one device round trip.  What it returns is what rp_check.h, rp_ensemble.h, rp_clearance.h and rp_score.h take.
 * rp_lift_points is the bare batch form of CoordinateSystem.convert_to_cartesian_coords.
 *
 * A lifter shares nothing with a planning context (rp_ctx), the checkers or the scorer: it owns its stream, its segment table and
 * its buffers, and all of them can live side by side in a process.  Built from csrc/rp_lift.hip alone; the other libraries are not
 * touched by it.
 *
 * Conventions: those of rp_score.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that are only read or
 * written during the call, 0 or a negative RP_E* code as the return value, the message from rp_lift_last_error, nothing throws
 * across the ABI.  Calls on one object must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (params->struct_size is not this library's
 * sizeof), RP_ESTATE (no reference was ever set, or the object has no device: rp_lift_create had failed), RP_ENOMEM, RP_EHIP
 * (a HIP call failed; the message has its text).
 * Every entry that takes an rp_lift makes the object's device the calling thread's current HIP device (hipSetDevice) and leaves
 * it so.
 */
#ifndef RP_LIFT_H
#define RP_LIFT_H

#include "rp_amd.h" /* rp_params, RP_E*, RP_STATUS_*, RP_REASON_*, RP_CHECK_* */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_LIFT_ABI_VERSION 1

typedef struct rp_lift rp_lift;

int rp_lift_abi_version(void);
/* *out is set even when the call fails (rp_lift_last_error then has the reason; destroy it all the same). */
int rp_lift_create(rp_lift **out, int device);
void rp_lift_destroy(rp_lift *lf);
const char *rp_lift_last_error(const rp_lift *lf);

/* The tables of rp_build_reference: n vertices ref_xy[n][2], their arc lengths ref_pos[n], the UNWRAPPED orientations
 * ref_theta[n], the curvature ref_curv[n] and its derivative ref_curv_d[n]; proj_domain_d_limit: |d| beyond which a pose has no
 * Cartesian position.  Builds one row per segment k on the host -- p0, e = p1 - p0, t0, t1 - t0 (unit vertex tangents: normalised
 * sum of the two adjacent unit segment directions), pos0, pos1 - pos0, theta0, theta1 - theta0, curv0, curv1 - curv0, curv_d0,
 * curv_d1 - curv_d0 -- uploads the rows and replaces the table of an earlier call.
 * RP_EINVAL: n < 2; a null table; a non-finite value; ref_pos not strictly increasing; a zero-length segment;
 * proj_domain_d_limit not positive (or not finite). */
int rp_lift_set_reference(rp_lift *lf, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta,
                          const double *ref_curv, const double *ref_curv_d, double proj_domain_d_limit);

/* Most poses (points) of one call: beyond it the call is refused with RP_EINVAL. */
#define RP_LIFT_MAX_POSES ((int64_t)1 << 24)

/* THE SEGMENT AND ON-PATH RULE, that of CoordinateSystem.convert_to_cartesian_coords.  The segment of s is k = the last vertex
 * with ref_pos[k] <= s, clamped to n - 2 (s == ref_pos[n-1] lies on the last segment, at lambda = 1); lambda = (s - pos0) / (pos1 -
 * pos0).  s is ON THE PATH when it is finite and ref_pos[0] <= s <= ref_pos[n-1]; a POSE is on the path when its s is, its d is
 * finite and |d| <= proj_domain_d_limit.  The position of a pose on the path is x = px - d * (ty / |t|), y = py + d * (tx / |t|)
 * with p = p0 + lambda e and t = t0 + lambda (t1 - t0).
 * The reference planner's kinematic loop (reactive_planner.py:835) instead takes np.argmax(ref_pos > s) - 1, which wraps to the
 * table's last index for s < ref_pos[0] and for s == ref_pos[n-1]: there it interpolates between the last and the first vertex or
 * drops the trajectory.  THAT QUIRK IS NOT KEPT: the rule above holds for the orientation, the curvature and the position alike.
 *
 * n_points points s[], d[]; x[], y[] receive the positions (NaN off the path), segment[] the index k (-1 off the path),
 * *n_outside the number of points off the path, counted on the device.
 * RP_EINVAL: n_points < 0 or > RP_LIFT_MAX_POSES; null s or d with n_points > 0.  RP_ESTATE: no reference set.
 * n_points == 0 succeeds with *n_outside = 0. */
int rp_lift_points(rp_lift *lf, int64_t n_points, const double *s, const double *d, double *x, double *y, int32_t *segment,
                   int64_t *n_outside);

/* K trajectories of up to n_poses poses each: the six input planes s, s_dot, s_ddot, d, d_dot, d_ddot are [K][n_poses]; len[k]
 * (1 <= len[k] <= n_poses) is the number of valid poses of trajectory k, len == NULL: n_poses for all; theta0[k] is the global
 * orientation trajectory k starts with (read by the standstill rule below), theta0 == NULL: params->x0_orientation for all.  Of
 * params the call reads struct_size, dt, low_vel_mode, constraint_mask, wheelbase, a_max, v_switch, delta_max, v_delta_max and
 * x0_orientation.  flags is reserved and must be 0.  In low-velocity mode d_dot and d_ddot are derivatives with respect to s.
 *
 * Per pose i < len[k], as ReactivePlanner._check_kinematics does (reactive_planner.py:776-896):
 *   |s_dot| < 1e-5 becomes 0 and |d_dot| < 1e-5 becomes 0.
 *   High-velocity mode: d' = d_dot / s_dot and d'' = (d_ddot - d' s_ddot) / s_dot^2 where s_dot > 0.001, both 0 otherwise.
 *   Low-velocity mode: d' = d_dot, d'' = d_ddot.
 *   With th_r = theta0 + lambda (theta1 - theta0) of the segment wrapped into [-pi, pi) (interpolate_angle):
 *     a moving pose (s_dot > 0.001) and every pose in low-velocity mode: theta_cl = atan2(d', 1), theta = theta_cl + th_r;
 *     a pose at standstill in high-velocity mode (s_dot <= 0.001) keeps the global orientation: theta[i] = theta[i-1], theta[0] =
 *     theta0[k], and theta_cl = theta - th_r, NOT wrapped, as the reference leaves it.  |theta_cl| is expected below 1e5 rad.
 *   With k_r and k_r' interpolated at lambda, q = 1 - k_r d, c = cos(theta_cl), t = tan(theta_cl):
 *     kappa = (d'' + (k_r d' + k_r' d) t) c (c / q)^2 + (c / q) k_r
 *     v = s_dot (q / c)
 *     a = s_ddot q / c + (s_dot^2 / c) (q t (kappa q / c - k_r) - (k_r' d + k_r d'))
 *   kappa_dot[i] = kappa[i] - kappa[i-1], kappa_dot[0] = 0: the unscaled first difference the reference stores.
 *   x, y: as rp_lift_points gives them.
 *
 * The verdict, in the reference's order.  The steps are walked in ascending order.  A step whose s is off the path, or one of
 * whose six inputs is not finite, stops the trajectory there with RP_REASON_OUT_OF_DOMAIN.  Otherwise the enabled checks run in
 * the order and with the arithmetic rp_score.h documents -- velocity (v < -1e-5), kappa (|kappa| > tan(delta_max) / wheelbase), yaw
 * rate (|rint((theta[i] - theta[i-1]) / dt * 1e5) / 1e5| > kappa_max v), kappa_dot (|(kappa[i] - kappa[i-1]) / dt| > v_delta_max (1
 * + (wheelbase kappa)^2) / wheelbase), acceleration (not -a_max <= a <= a_max, or a_max v_switch / v above v_switch); both rates
 * are 0 at i = 0.  The first failing step decides, then the first failing check at that step.  A trajectory that passes every step
 * but has a pose with |d| > proj_domain_d_limit gets RP_REASON_OUT_OF_DOMAIN at the first such pose.  No pre-filter, no horizon
 * extension: the reference's draw-mode loop over the trajectory's own length.
 *   status[k]: label | reason << 4 | step << 8 as RP_STATUS_LABEL / REASON / STEP of rp_amd.h, the label RP_LABEL_FEASIBLE or
 *     RP_LABEL_INFEASIBLE_KINEMATIC (out of domain as well); a step beyond 4095 is reported as 4095.
 *
 * Outputs, each [K][n_poses]: x, y, theta, v, a, kappa, kappa_dot, theta_cl.  From the first pose that stops the trajectory
 * onward every plane is NaN; a pose with |d| > proj_domain_d_limit has NaN x and y only; poses i >= len[k] are NaN.  A trajectory
 * infeasible for a kinematic reason still gets all its rows, as in draw mode.
 *   *first_feasible: the smallest feasible k, -1 if none; *n_feasible; reason_counts[8]: trajectories per RP_REASON_* (1 .. 6; 0
 *   and 7 stay 0).  All reduced on the device.
 * Every output pointer may be NULL.
 * RP_EINVAL: K < 0; n_poses < 1; K or K * n_poses > RP_LIFT_MAX_POSES; a len[k] out of range; a null input plane with K > 0; dt
 *   not positive; unknown flags.
 * RP_EABI: params->struct_size.  RP_ESTATE: no reference set (checked before K == 0 returns).
 * K == 0 succeeds with *first_feasible = -1, *n_feasible = 0 and zero counts. */
int rp_lift_evaluate(rp_lift *lf, const rp_params *params, int64_t K, int32_t n_poses, const double *s, const double *s_dot,
                     const double *s_ddot, const double *d, const double *d_dot, const double *d_ddot, const int32_t *len,
                     const double *theta0, uint32_t flags, double *x, double *y, double *theta, double *v, double *a, double *kappa,
                     double *kappa_dot, double *theta_cl, uint32_t *status, int64_t *first_feasible, int64_t *n_feasible,
                     int64_t *reason_counts);

#ifdef __cplusplus
}
#endif
#endif /* RP_LIFT_H */
