/*
 * rp_pick.h -- C ABI of the pick among curvilinear trajectories the caller brings (librp_pick.so).
 *
 * rp_plan* picks the cheapest feasible, collision-free candidate of the planner's own polynomial grid.  rp_lift.h, rp_score.h and
 * rp_check.h answer one question each for trajectories the caller brings, and a caller who wanted the planner's DECISION for such a
 * bundle chained them through host memory: lift, cost and argsort on the host, poses back to the device for the check, first_free
 * mapped back.  This library is that chain as one call: K given trajectories s, s', s'', d, d', d'' along a reference path -- a
 * lateral QP's output, a corridor optimiser's, a learned Frenet proposal -- become, in one device round trip,
 *   per trajectory the status word, the cost and the first colliding pose / segment,
 *   per call what ReactivePlanner._get_optimal_trajectory decides: the cheapest kinematically feasible, collision-free trajectory,
 *   the reference planner's statistics, and the winner's full state block.
 * No pose plane goes through host memory unless the caller asks for it.
 *
 * A picker shares nothing with a planning context (rp_ctx), the lifter, the checkers or the scorer: it owns its stream, its
 * segment table, its obstacle tables and its buffers, and all of them can live side by side in a process.  Built from
 * csrc/rp_pick.hip and the source files that state the lift step and the obstacle walk for the lifter and the checker as well; the
 * other libraries compute what they computed.  The rules it applies are not restated here: the headers named with each of them
 * define them.
 *
 * Conventions: those of rp_lift.h -- plain pointers and sizes, caller-owned C-contiguous host buffers that are only read or
 * written during the call, 0 or a negative RP_E* code as the return value, the message from rp_pick_last_error, nothing throws
 * across the ABI.  Calls on one object must be serialised by the caller.
 * Return codes besides RP_OK: RP_EINVAL (arguments, listed with each call), RP_EABI (a struct_size is not this library's sizeof),
 * RP_ESTATE (no reference was ever set, or the object has no device: rp_pick_create had failed), RP_ENOMEM, RP_EHIP (a HIP call
 * failed; the message has its text).
 * Every entry that takes an rp_pick makes the object's device the calling thread's current HIP device (hipSetDevice) and leaves
 * it so.
 */
#ifndef RP_PICK_H
#define RP_PICK_H

#include "rp_amd.h"   /* rp_params, rp_cost, RP_E*, RP_STATUS_*, RP_LABEL_*, RP_REASON_*, RP_CHECK_*, RP_COST_*, enum rp_array */
#include "rp_check.h" /* RP_TRAJ_POSES, RP_TRAJ_SWEPT */

#ifdef __cplusplus
extern "C" {
#endif

#define RP_PICK_ABI_VERSION 1

typedef struct rp_pick rp_pick;

int rp_pick_abi_version(void);
/* *out is set even when the call fails (rp_pick_last_error then has the reason; destroy it all the same). */
int rp_pick_create(rp_pick **out, int device);
void rp_pick_destroy(rp_pick *pk);
const char *rp_pick_last_error(const rp_pick *pk);

/* The segment table: the arguments, the rows and the refusals of rp_lift_set_reference (rp_lift.h).  A refused table leaves the
 * earlier one in place. */
int rp_pick_set_reference(rp_pick *pk, int32_t n, const double *ref_xy, const double *ref_pos, const double *ref_theta,
                          const double *ref_curv, const double *ref_curv_d, double proj_domain_d_limit);

/* The obstacle tables: the arguments, the meaning and the refusals of rp_checker_set_obstacles (rp_check.h).  A picker that was
 * never given tables checks against empty ones.  A refused table leaves the earlier ones in place. */
int rp_pick_set_obstacles(rp_pick *pk, int32_t n_sobb, const double *sobb, int32_t n_tri, const double *tri, int32_t n_circ,
                          const double *circ, int32_t n_dyn, int32_t n_steps, int32_t dyn_t0, const double *dyn);

/* Most poses of one call: beyond it the call is refused with RP_EINVAL. */
#define RP_PICK_MAX_POSES ((int64_t)1 << 24)

/* The scalars of a call, all reduced on the device. */
typedef struct rp_pick_result {
    uint32_t struct_size;            /* sizeof(rp_pick_result), set by the caller: RP_EABI on a mismatch */
    uint32_t reserved_;
    int64_t best;                    /* the lexicographic minimum of (cost, k) over the trajectories with RP_LABEL_FEASIBLE; -1: none */
    double best_cost;                /* its cost; NaN: none */
    int64_t n_feasible;              /* kinematically feasible trajectories, colliding ones included: K - n_feasible is the
                                        reference's infeasible_count_kinematics */
    int64_t n_collision;             /* kinematically feasible trajectories with a hit in a requested test */
    int64_t n_collision_before_best; /* those of them with (cost, k) below the winner's, all of them when there is no winner: the
                                        reference's _infeasible_count_collision of the sorted walk */
    int64_t reason_counts[8];        /* trajectories per RP_REASON_* (1 .. 6; 0 and 7 stay 0), as rp_lift_evaluate gives them */
} rp_pick_result;
#define RP_PICK_RESULT_INIT {(uint32_t)sizeof(rp_pick_result)}

/* K trajectories of up to n_poses poses each.  The six input planes, len, theta0 and the eight output planes x .. theta_cl are
 * those of rp_lift_evaluate (rp_lift.h) and mean what they mean there; of params the call reads what rp_lift_evaluate and
 * rp_checker_check read, of cost everything.  flags is reserved and must be 0.
 *
 * Per pose and kinematic verdict: rp_lift_evaluate, exactly -- the segment and on-path rule, the standstill rule with theta0,
 *   low-velocity mode, the order of the checks, RP_REASON_OUT_OF_DOMAIN for an off-path or non-finite step and, behind every step's
 *   own failure, for |d| beyond the limit, and the NaN pattern of the eight planes.
 * cost_out[k]: DefaultCostFunction (RP_COST_DEFAULT) or DefaultCostFunctionFailSafe (RP_COST_FAILSAFE) as rp_score.h states
 *   them, over the len[k] poses with the given s and d and the lifted v, a and theta_cl: the last entry is pose len[k] - 1, the
 *   middle entry v[len[k] / 2]; no horizon extension.  NaN for a kinematically infeasible trajectory.
 * Collision: mode is any of RP_TRAJ_POSES | RP_TRAJ_SWEPT (rp_check.h); 0: no collision test.  Every kinematically feasible
 *   trajectory is tested, eagerly, on the lifted x, y, theta of this call, with the ego rectangles, time indices (time_step0 + i *
 *   factor for poses, time_step0 + i for segments), absent rows and indices outside the table of rp_checker_check.
 *   first_pose_hit[k] / first_segment_hit[k]: the smallest colliding index, -1 if none -- and -1 for a trajectory that is not
 *   kinematically feasible, which is not tested.
 * status[k]: RP_LABEL_FEASIBLE -- feasible and free in every requested test;
 *   RP_LABEL_INFEASIBLE_KINEMATIC | reason << 4 | step << 8 as rp_lift_evaluate gives it;
 *   RP_LABEL_INFEASIBLE_COLLISION | 0 << 4 | step << 8 with step = the first colliding pose if the pose test hit, else the first
 *   colliding segment, reported as 4095 beyond it.
 * result: see rp_pick_result.  A NaN cost never wins.
 * best_states [RP_N_ARRAYS][n_poses]: the winner's rows in the order of enum rp_array -- x .. kappa_dot and theta_cl from the
 *   device, s, d and their four derivatives the inputs --, NaN beyond len[best], NaN everywhere when there is no winner.  Its rows
 *   are bit-equal to the planes of the same call.
 * Every output pointer may be NULL, and which outputs are asked for never changes any other output.
 * RP_EINVAL: what rp_lift_evaluate refuses (K < 0; n_poses < 1; K or K * n_poses > RP_PICK_MAX_POSES; a len[k] out of range; a
 *   null input plane with K > 0; dt not positive; unknown flags) and what rp_checker_check refuses (an unknown mode bit;
 *   first_pose_hit without RP_TRAJ_POSES or first_segment_hit without RP_TRAJ_SWEPT); null params or cost; cost->kind not
 *   RP_COST_DEFAULT or RP_COST_FAILSAFE (RP_COST_EXTERNAL included); a non-NaN desired_speed / desired_d / desired_s that is not
 *   finite.
 * RP_EABI: params->struct_size, cost->struct_size or result->struct_size.  RP_ESTATE: no reference set (checked before K == 0
 * returns).
 * K == 0 succeeds with best = -1, best_cost = NaN and zero counts. */
int rp_pick_select(rp_pick *pk, const rp_params *params, const rp_cost *cost, uint32_t mode, int64_t K, int32_t n_poses,
                   const double *s, const double *s_dot, const double *s_ddot, const double *d, const double *d_dot,
                   const double *d_ddot, const int32_t *len, const double *theta0, uint32_t flags,
                   /* per pose, each [K][n_poses], each may be NULL */
                   double *x, double *y, double *theta, double *v, double *a, double *kappa, double *kappa_dot, double *theta_cl,
                   /* per trajectory, each may be NULL */
                   uint32_t *status, double *cost_out, int32_t *first_pose_hit, int32_t *first_segment_hit,
                   /* per call, each may be NULL */
                   rp_pick_result *result, double *best_states /* [RP_N_ARRAYS][n_poses] */);

#ifdef __cplusplus
}
#endif
#endif /* RP_PICK_H */
