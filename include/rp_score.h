/*
 * rp_score.h -- C ABI of the scorer for trajectories the caller brings (librp_score.so).
 *
 * rp_check.h, rp_ensemble.h and rp_clearance.h answer the collision third of what the planner does with a candidate.  This
 * library answers the other two thirds for K GIVEN trajectories -- Cartesian poses from anywhere: last cycle's winner shifted by
 * a step, an optimiser's output, a learned proposal, an obstacle's predicted path -- in one device round trip:
 *   their curvilinear coordinates s, d, theta_cl along a reference path (the batch form of rp_project),
 *   the reference planner's kinematic verdict (ReactivePlanner._check_constraints),
 *   the reference planner's default cost (DefaultCostFunction / DefaultCostFunctionFailSafe),
 *   and the cheapest feasible one.
 * rp_score_project is the bare batch projection of points.
 *
 * A scorer shares nothing with a planning context (rp_ctx) or the checkers: it owns its stream, its segment table and its pose
 * and result buffers, and all of them can live side by side in a process.  Built from csrc/rp_score.hip alone; the other
 * libraries are not touched by it.
 *
 * Conventions: those of rp_clearance.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that are only read or
 * written during the call, 0 or a negative RP_E* code as the return value, the message from rp_score_last_error, nothing throws
 * across the ABI.  Calls on one object must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (a struct_size is not this library's
 * sizeof), RP_ESTATE (no reference was ever set, or the object has no device: rp_score_create had failed), RP_ENOMEM, RP_EHIP
 * (a HIP call failed; the message has its text).
 * Every entry that takes an rp_score makes the object's device the calling thread's current HIP device (hipSetDevice) and
 * leaves it so.
 */
#ifndef RP_SCORE_H
#define RP_SCORE_H

#include "rp_amd.h" /* rp_params, rp_cost, RP_E*, RP_STATUS_*, RP_REASON_*, RP_CHECK_*, RP_COST_* */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_SCORE_ABI_VERSION 1

typedef struct rp_score rp_score;

int rp_score_abi_version(void);
/* *out is set even when the call fails (rp_score_last_error then has the reason; destroy it all the same). */
int rp_score_create(rp_score **out, int device);
void rp_score_destroy(rp_score *sc);
const char *rp_score_last_error(const rp_score *sc);

/* The tables of rp_set_reference / rp_build_reference: n vertices ref_xy[n][2], their arc lengths ref_pos[n] and the UNWRAPPED
 * orientations ref_theta[n] (as rp_build_reference returns them); proj_domain_d_limit: |d| beyond which a point is outside
 * the projection domain.  Builds one row per segment k on the host -- p0, e = p1 - p0, t0, t1 - t0 (unit vertex tangents:
 * normalised sum of the two adjacent unit segment directions), pos0, pos1 - pos0, theta0, theta1 - theta0 -- uploads the rows and
 * replaces the table of an earlier call.
 * RP_EINVAL: n < 2; a non-finite value; ref_pos not strictly increasing; a zero-length segment; proj_domain_d_limit not
 * positive (or not finite). */
int rp_score_set_reference(rp_score *sc, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta,
                           double proj_domain_d_limit);

/* Most poses (points) of one call: beyond it the call is refused with RP_EINVAL. */
#define RP_SCORE_MAX_POSES ((int64_t)1 << 24)

/* flags of rp_score_evaluate */
#define RP_SCORE_EXHAUSTIVE (1u << 0) /* walk every segment for every pose, no pruning: a diagnostic, results do not depend on it */

/* THE PROJECTION (x, y) -> (s, d, segment), the definition of rp_project stated precisely.  Segments are walked in ascending
 * index.  On segment k the foot point p0 + lam e solves ((P - p0) - lam e) . (t0 + lam (t1 - t0)) = 0, a quadratic a lam^2 + b lam
 * + c with a = -e . dt, b = q . dt - e . t0, c = q . t0 (q = P - p0, dt = t1 - t0): for |a| < 1e-14 the one root -c / b (none when
 * b == 0); otherwise none when the discriminant is negative, else with h = -(b + sqrt(disc)) / 2 for b >= 0 the roots c / h, h / a
 * in that order, with h = -(b - sqrt(disc)) / 2 for b < 0 the roots h / a, c / h in that order (h == 0: the root 0).  A root is
 * admissible when it lies in [-1e-12, 1 + 1e-12]; it is then clamped to [0, 1].  Its d is the offset of P from the foot point
 * along the normalised tangent t0 + lam dt rotated by +90 degrees; it is a candidate when |d| <= proj_domain_d_limit.  A
 * candidate replaces the held one only when its |d| is STRICTLY smaller: the first segment wins an exact tie.
 * s = pos0 + lam (pos1 - pos0).  A point without a candidate (a NaN coordinate included) is outside the projection domain.
 *
 * n_points points x[], y[]; s[], d[] receive the coordinates (NaN outside the domain), segment[] the index of the segment
 * that was chosen (-1 outside), *n_outside the number of points outside, counted on the device.
 * RP_EINVAL: n_points < 0 or > RP_SCORE_MAX_POSES; null x or y with n_points > 0.  RP_ESTATE: no reference set.
 * n_points == 0 succeeds with *n_outside = 0. */
int rp_score_project(rp_score *sc, int64_t n_points, const double *x, const double *y, double *s, double *d, int32_t *segment,
                     int64_t *n_outside);

/* K trajectories of up to n_poses rear-axle poses each: x, y, theta, v, a, kappa are [K][n_poses]; len[k] (1 <= len[k] <=
 * n_poses) is the number of valid poses of trajectory k, len == NULL: n_poses for all.  v, a and kappa may be NULL where nothing
 * reads them (below).  Of params the call reads struct_size, dt, constraint_mask, wheelbase, a_max, v_switch, delta_max and
 * v_delta_max; of cost everything.  Only poses i < len[k] take part in anything.
 *   s_out, d_out, theta_cl_out [K][n_poses]: the projection of every pose (above), theta_cl = theta - (theta0 + lam (theta1 -
 *     theta0)) wrapped into [-pi, pi) (make_valid_orientation); NaN outside the domain and for i >= len[k].
 *   Kinematics: ReactivePlanner._check_constraints on the caller's v, kappa, theta, a.  Per step the enabled checks run in the
 *     order velocity (v < -1e-5), kappa (|kappa| > tan(delta_max) / wheelbase), yaw rate (|round((theta[i] - theta[i-1]) / dt,
 *     5)| > kappa_max v, round = rint(x * 1e5) / 1e5), kappa_dot (|(kappa[i] - kappa[i-1]) / dt| > v_delta_max (1 + (wheelbase
 *     kappa)^2) / wheelbase), acceleration (not -a_max <= a <= a_max, or a_max v_switch / v above v_switch); both rates are 0 at
 *     i = 0.  The first failing step, then the first failing check at that step, decides.  A trajectory that passes them but has a
 *     pose outside the projection domain gets RP_REASON_OUT_OF_DOMAIN at the first such pose (the reference's order: the whole
 *     kinematic loop runs before the positions).
 *   status[k]: label | reason << 4 | step << 8 as RP_STATUS_LABEL / REASON / STEP of rp_amd.h, the label RP_LABEL_FEASIBLE or
 *     RP_LABEL_INFEASIBLE_KINEMATIC (out of domain as well); a step beyond 4095 is reported as 4095.
 *   cost[k]: DefaultCostFunction.evaluate (RP_COST_DEFAULT: w_a, desired_speed, desired_d, desired_s; NaN = None) or
 *     DefaultCostFunctionFailSafe.evaluate (RP_COST_FAILSAFE) over the len[k] poses with the projected s, d, theta_cl and the
 *     given v, a: the last entry is pose len[k] - 1, the middle entry v[len[k] / 2]; no horizon extension.  NaN for an infeasible
 *     trajectory.
 *   *best: the lexicographic minimum of (cost, k) over the feasible trajectories, -1 if there is none (a NaN cost never wins);
 *     *best_cost: its cost, NaN if none; *n_feasible; reason_counts[8]: trajectories per RP_REASON_* (1 .. 6; 0 and 7 stay 0).
 *     All reduced on the device.
 * Every output pointer may be NULL.
 * RP_EINVAL: K < 0; n_poses < 1; K or K * n_poses > RP_SCORE_MAX_POSES; a len[k] out of range; null x, y or theta with K > 0;
 *   dt not positive; constraint_mask asks for a check whose array is NULL (velocity: v; kappa, kappa_dot: kappa; yaw rate: v;
 *   acceleration: a and v); a == NULL; desired_speed set (RP_COST_DEFAULT) and v == NULL; cost->kind not RP_COST_DEFAULT or
 *   RP_COST_FAILSAFE; a non-NaN desired_speed / desired_d / desired_s that is not finite; unknown flags.
 * RP_EABI: params->struct_size or cost->struct_size.  RP_ESTATE: no reference set (checked before K == 0 returns).
 * K == 0 succeeds with *best = -1, *best_cost = NaN, *n_feasible = 0 and zero counts. */
int rp_score_evaluate(rp_score *sc, const rp_params *params, const rp_cost *cost, int64_t K, int32_t n_poses, const double *x,
                      const double *y, const double *theta, const double *v, const double *a, const double *kappa,
                      const int32_t *len, uint32_t flags, double *s_out, double *d_out, double *theta_cl_out, uint32_t *status,
                      double *cost_out, int64_t *best, double *best_cost, int64_t *n_feasible, int64_t *reason_counts);

#ifdef __cplusplus
}
#endif
#endif /* RP_SCORE_H */
