// rp_pick_cost.h -- the cost of a given trajectory as include/rp_pick.h states it, stated once: the cost's scalars on the device, the
// host's reading of an rp_cost into them and the terms one pose adds.  Included by rp_pick.hip (librp_pick.so) and rp_epick.hip
// (librp_epick.so); everything here has internal linkage, nothing of it is exported by either.
#ifndef RP_PICK_COST_H
#define RP_PICK_COST_H

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/rp_amd.h"

namespace {

// cost_function.py:51-71, 82-92 as rp_score.hip holds it: the fail-safe cost is the default one with w_a = 1, desired_d = 0 and no
// v / s terms
struct PkCost {
    int32_t has_speed, has_s;
    double w_a, desired_speed, desired_d, desired_s;
};

// The terms of pose i, added to `sum` in this order: a lane calls it for its poses in ascending order.  last: the trajectory's last
// pose, mid: its middle one.  (A closure over the walking kernel's own variables, as the lambda was that stood in rp_pick.hip.)
struct PkAddCost {
    const PkCost &cc;
    double &sum;
    const int &last, &mid;
    __device__ void operator()(int i, double vel, double acc, double thcl, double s, double d) const {
        const double th = fabs(thcl);
        double e;
        e = cc.w_a * acc; sum += e * e;
        e = 0.25 * (cc.desired_d - d); sum += e * e;
        e = 0.25 * th; sum += e * e;
        if (cc.has_speed) { e = 5.0 * (vel - cc.desired_speed); sum += e * e; }
        if (cc.has_s) { e = 0.25 * (cc.desired_s - s); sum += e * e; }
        if (i == last) {
            e = 20.0 * (cc.desired_d - d); sum += e * e;
            e = 5.0 * th; sum += e * e;
            if (cc.has_speed) { e = vel - cc.desired_speed; sum += 50.0 * (e * e); }
            if (cc.has_s) { e = 20.0 * (cc.desired_s - s); sum += e * e; }
        }
        if (i == mid && cc.has_speed) { e = vel - cc.desired_speed; sum += 100.0 * (e * e); }
    }
};

// an rp_cost the call has accepted (kind RP_COST_DEFAULT or RP_COST_FAILSAFE) as the device reads it
inline PkCost pk_cost_of(const rp_cost *cost) {
    const bool failsafe = cost->kind == RP_COST_FAILSAFE;
    const bool has_speed = !failsafe && !std::isnan(cost->desired_speed), has_s = !failsafe && !std::isnan(cost->desired_s);
    return {has_speed ? 1 : 0, has_s ? 1 : 0, failsafe ? 1.0 : cost->w_a, has_speed ? cost->desired_speed : 0.0, failsafe ? 0.0 : cost->desired_d,
            has_s ? cost->desired_s : 0.0};
}

}  // namespace

#endif  // RP_PICK_COST_H
