/*
 * rp_epick.h -- C ABI of the pick among curvilinear trajectories the caller brings, under a bound on the collision risk over M
 * sampled predictions of the dynamic obstacles (librp_epick.so).
 *
 * rp_pick.h gives the planner's decision for K given trajectories against ONE table of dynamic obstacles.  rp_ensemble.h tests K
 * given poses against M sampled futures ("members") and knows nothing of feasibility or cost.  A caller who plans against uncertain
 * predictions wants the cheapest kinematically feasible trajectory whose collision risk over the M futures stays under a bound, and
 * chained the two through host memory: rp_pick_select without a test for x, y and theta, rp_ensemble_check on the feasible rows, the
 * member weights, the mask and the minimum on the host.  This library is that chain as one call: K given trajectories s, s', s'', d,
 * d', d'' along a reference path become, in one device round trip,
 *   per trajectory the status word, the cost, the members it collides in, the sum of their weights (the "risk") and per member the
 *   first colliding pose / segment,
 *   per call the cheapest kinematically feasible trajectory whose risk is at most the bound, the statistics of rp_pick_select and the
 *   winner's full state block, its member count and its risk.
 * No pose plane goes through host memory unless the caller asks for it.
 *
 * An rp_epick shares nothing with a planning context (rp_ctx), the lifter, the checkers, the scorer or the picker: it owns its
 * stream, its segment table, its obstacle tables and its buffers, and all of them can live side by side in a process.  Built from
 * csrc/rp_epick.hip and the source files that state the lift step, the obstacle walk and the cost for the lifter, the checker and the
 * picker as well; the other libraries compute what they computed.  The rules it applies are not restated here: the headers named with
 * each of them define them.
 *
 * Conventions: those of rp_pick.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that are only read or written
 * during the call, 0 or a negative RP_E* code as the return value, the message from rp_epick_last_error, nothing throws across the
 * ABI.  Calls on one object must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (a struct_size is not this library's sizeof),
 * RP_ESTATE (no reference was ever set, or the object has no device: rp_epick_create had failed), RP_ENOMEM, RP_EHIP (a HIP call
 * failed; the message has its text).
 * Every entry that takes an rp_epick makes the object's device the calling thread's current HIP device (hipSetDevice) and leaves it
 * so.
 */
#ifndef RP_EPICK_H
#define RP_EPICK_H

#include "rp_amd.h"   /* rp_params, rp_cost, RP_E*, RP_STATUS_*, RP_LABEL_*, RP_REASON_*, RP_CHECK_*, RP_COST_*, enum rp_array */
#include "rp_check.h" /* RP_TRAJ_POSES, RP_TRAJ_SWEPT */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_EPICK_ABI_VERSION 1

typedef struct rp_epick rp_epick;

int rp_epick_abi_version(void);
/* *out is set even when the call fails (rp_epick_last_error then has the reason; destroy it all the same).
 * A fresh object has no static shapes and one member of weight 1 without dynamic obstacles. */
int rp_epick_create(rp_epick **out, int device);
void rp_epick_destroy(rp_epick *ep);
const char *rp_epick_last_error(const rp_epick *ep);

/* The segment table: the arguments, the rows and the refusals of rp_lift_set_reference (rp_lift.h).  A refused table leaves the
 * earlier one in place. */
int rp_epick_set_reference(rp_epick *ep, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta,
                           const double *ref_curv, const double *ref_curv_d, double proj_domain_d_limit);

/* Most members, most dynamic rows of all members together (n_members * n_dyn * n_steps), most poses of one call (K * n_poses) and
 * most verdicts of one call (K * n_members), the values of rp_ensemble.h: beyond any of them a call is refused with RP_EINVAL. */
#define RP_EPICK_MAX_MEMBERS 4096
#define RP_EPICK_MAX_DYN_ROWS ((int64_t)1 << 22)
#define RP_EPICK_MAX_POSES ((int64_t)1 << 24)
#define RP_EPICK_MAX_VERDICTS ((int64_t)1 << 24)

/* The static shapes: the arguments, the meaning and the refusals of rp_ensemble_set_static (rp_ensemble.h).  They do not depend on
 * the member: a hit on one of them counts in every member.  Replaces the static shapes of an earlier call and leaves the members as
 * they are.  A refused table leaves the earlier shapes in place. */
int rp_epick_set_static(rp_epick *ep, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ,
                        const double *circ);

/* dyn[n_members][n_dyn][n_steps][5], dyn_t0: the members' tables, their limits and their refusals as rp_ensemble_set_members has
 * them (n_members < 1 or > RP_EPICK_MAX_MEMBERS; a negative count; n_members * n_dyn * n_steps > RP_EPICK_MAX_DYN_ROWS; null dyn
 * with rows).  weight[n_members]: what member m adds to the risk of a trajectory that collides in it; NULL: every weight is 1.0.  A
 * negative or non-finite weight: RP_EINVAL.  The tables and the weights go to the device here, not with every rp_epick_select.
 * Replaces the members and the weights of an earlier call and leaves the static shapes as they are.  A refused call leaves the
 * earlier members and weights in place. */
int rp_epick_set_members(rp_epick *ep, int32_t n_members, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn,
                         const double *weight);

/* The scalars of a call, all reduced on the device: the fields of rp_pick_result (rp_pick.h), then the winner's two. */
typedef struct rp_epick_result {
    uint32_t struct_size;            /* sizeof(rp_epick_result), set by the caller: RP_EABI on a mismatch */
    uint32_t reserved_;
    int64_t best;                    /* the lexicographic minimum of (cost, k) over the trajectories with RP_LABEL_FEASIBLE; -1: none */
    double best_cost;                /* its cost; NaN: none */
    int64_t n_feasible;              /* kinematically feasible trajectories, those over the bound included */
    int64_t n_collision;             /* kinematically feasible trajectories with risk[k] > max_risk */
    int64_t n_collision_before_best; /* those of them with (cost, k) below the winner's, all of them when there is no winner */
    int64_t reason_counts[8];        /* trajectories per RP_REASON_* (1 .. 6; 0 and 7 stay 0), as rp_lift_evaluate gives them */
    int64_t best_members_hit;        /* members_hit[best]; -1: none */
    double best_risk;                /* risk[best]; NaN: none */
} rp_epick_result;
#define RP_EPICK_RESULT_INIT {(uint32_t)sizeof(rp_epick_result)}

/* K trajectories of up to n_poses poses each, against the static shapes and the n_members members the object holds.  The six input
 * planes, len, theta0, flags, the eight output planes x .. theta_cl, params and cost are those of rp_pick_select (rp_pick.h).
 *
 * Per pose and kinematic verdict, the eight planes and their NaN pattern: rp_lift_evaluate (rp_lift.h), exactly.
 * cost_out[k]: rp_pick_select, exactly.
 * Collision: mode is any of RP_TRAJ_POSES | RP_TRAJ_SWEPT (rp_check.h); 0: no collision test.  Every kinematically feasible
 *   trajectory is tested, eagerly, in every member, on the lifted x, y, theta of this call, with the ego rectangles, time indices
 *   (time_step0 + i * factor for poses, time_step0 + i for segments), absent rows and indices outside the table of rp_checker_check.
 *   The verdict per (k, m) is what rp_checker_check gives on the static shapes and member m's table, hence what rp_ensemble_check
 *   gives; a static hit counts in every member.
 *   first_pose_hit[k][m] / first_segment_hit[k][m] ([K][n_members]): the smallest colliding index, -1 if none -- and a whole row of -1
 *   for a trajectory that is not kinematically feasible, which is not tested.
 * members_hit[k]: the members in which trajectory k has a hit in a requested test.
 * risk[k]: the sum of weight[m] over those members, added in double, in ascending m, one after the other, starting from 0.0 (the
 *   order is part of the ABI: the same bits for any weights).  With NULL weights it equals members_hit[k] exactly.  Both are 0 and 0.0
 *   for a trajectory that is not kinematically feasible, and for every trajectory when mode is 0.
 * status[k]: RP_LABEL_FEASIBLE -- kinematically feasible and risk[k] <= max_risk;
 *   RP_LABEL_INFEASIBLE_KINEMATIC | reason << 4 | step << 8 as rp_lift_evaluate gives it;
 *   RP_LABEL_INFEASIBLE_COLLISION | 0 << 4 | step << 8 -- kinematically feasible and risk[k] > max_risk -- with step = the smallest
 *   first_pose_hit[k][m] over the members if any member has a pose hit, else the smallest first_segment_hit[k][m], reported as 4095
 *   beyond it.  With one member this is rp_pick_select's word.
 * result: see rp_epick_result.  A NaN cost never wins.
 * best_states [RP_N_ARRAYS][n_poses]: as in rp_pick_select; its rows are bit-equal to the planes of the same call.
 * Every output pointer may be NULL, and which outputs are asked for never changes any other output.
 * RP_EINVAL: what rp_pick_select refuses (K < 0; n_poses < 1; K or K * n_poses > RP_EPICK_MAX_POSES; a len[k] out of range; a null
 *   input plane with K > 0; dt not positive; unknown flags; an unknown mode bit; first_pose_hit without RP_TRAJ_POSES or
 *   first_segment_hit without RP_TRAJ_SWEPT; null params or cost; cost->kind not RP_COST_DEFAULT or RP_COST_FAILSAFE; a non-NaN
 *   desired_speed / desired_d / desired_s that is not finite); K * n_members > RP_EPICK_MAX_VERDICTS; max_risk NaN or negative
 *   (+inf is allowed and accepts everything kinematically feasible).
 * RP_EABI: params->struct_size, cost->struct_size or result->struct_size.  RP_ESTATE: no reference set (checked before K == 0
 * returns).
 * K == 0 succeeds with best = -1, best_cost = NaN, best_members_hit = -1, best_risk = NaN and zero counts. */
int rp_epick_select(rp_epick *ep, const rp_params *params, const rp_cost *cost, uint32_t mode, double max_risk, int64_t K,
                    int32_t n_poses, const double *s, const double *s_dot, const double *s_ddot, const double *d,
                    const double *d_dot, const double *d_ddot, const int32_t *len, const double *theta0, uint32_t flags,
                    /* per pose, each [K][n_poses], each may be NULL */
                    double *x, double *y, double *theta, double *v, double *a, double *kappa, double *kappa_dot, double *theta_cl,
                    /* per trajectory, each may be NULL */
                    uint32_t *status, double *cost_out, int32_t *members_hit /* [K] */, double *risk /* [K] */,
                    int32_t *first_pose_hit /* [K][n_members] */, int32_t *first_segment_hit /* [K][n_members] */,
                    /* per call, each may be NULL */
                    rp_epick_result *result, double *best_states /* [RP_N_ARRAYS][n_poses] */);

#ifdef __cplusplus
}
#endif
#endif /* RP_EPICK_H */
