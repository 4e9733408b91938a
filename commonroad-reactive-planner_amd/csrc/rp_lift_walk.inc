// rp_lift_walk.inc -- the walk of ONE trajectory by one wavefront, 64 poses at a time, as TEXT: it is included inside the kernel
// that walks (the pose kernel of rp_lift.hip, the lift kernel of rp_pick.hip), so both compile the very same statements.
// In scope where it is included: tb (LfTable), kin (LfKin), row (LfRows), in (the six input planes, plane stride P, the trajectory's
// poses from in[base]), lane, k, L (its length), n (poses per row), theta0 (per trajectory, or nullptr).  It leaves `best`, the
// lane's smallest step << 3 | reason.  The includer says where a pose goes:
//   LF_PUT_NAN(i)                  pose i of a chunk behind the trajectory's end or behind the pose that stopped it: all NaN
//   LF_PUT_POSE(i, x, y, theta, v, a, kappa, kappa_dot, theta_cl, live, s, d)
//                                  pose i < n: the eight values as the planes hold them (NaN applied), whether the pose is one of the
//                                  trajectory in front of the pose that stops it, and the s and d the lane read for it
    const double nan = __builtin_nan("");
    const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;   // the lanes up to and including this one
    // what crosses a chunk boundary: the orientation a standstill keeps, theta and kappa of the chunk's last pose, and whether the
    // trajectory was stopped
    double keep = theta0 ? theta0[k] : kin.theta0, th_last = 0.0, kp_last = 0.0;
    bool dead = false;
    uint32_t best = LF_KEY_NONE;              // the lane's smallest step << 3 | reason
    const int nchunk = (n + 63) / 64;
    for (int c = 0; c < nchunk; ++c) {        // wave-uniform
        const int i = c * 64 + lane;
        if (c * 64 >= L || dead) {            // nothing but NaN from here on
            if (i < n) LF_PUT_NAN(i);
            continue;
        }
        const bool have = i < L;
        const size_t at = base + (size_t)(have ? i : 0);   // lanes behind the end: pose 0, never used
        const double s = in[at], sdd = in[2 * P + at], d = in[3 * P + at], ddd = in[5 * P + at];
        double sd = in[P + at], dd = in[4 * P + at];
        if (fabs(sd) < RP_EPS) sd = 0.0;
        if (fabs(dd) < RP_EPS) dd = 0.0;
        const bool on_s = lf_finite(s) && lf_finite(sd) && lf_finite(sdd) && lf_finite(d) && lf_finite(dd) && lf_finite(ddd) && s >= tb.pos_first && s <= tb.pos_last;
        const bool off = have && !on_s;
        const uint64_t offs = __ballot(off);
        const bool before = (offs & upto & ~(1ull << lane)) != 0;   // an earlier pose of this chunk stopped the trajectory
        const int seg = find_segment(row, tb.n_seg, tb.iters, s);
        const double pos0 = row(seg, R_POS), dpos = row(seg, R_DPOS);
        const double lam = (s - pos0) / dpos;
        const double th_r = make_valid_orientation(row(seg, R_DTH) * (s - pos0) / dpos + row(seg, R_TH));   // interpolate_angle
        const double kr = row(seg, R_DKR) * lam + row(seg, R_KR), krd = row(seg, R_DKRD) * lam + row(seg, R_KRD);
        const bool moving = sd > 0.001;
        double dp, dpp;
        if (kin.low_vel) { dp = dd; dpp = ddd; }
        else {
            dp = moving ? dd / sd : 0.0;
            dpp = moving ? (ddd - dp * sdd) / (sd * sd) : 0.0;
        }
        const bool stand = !kin.low_vel && !moving;
        const double thcl_m = rp_atan(dp);
        // The standstill carry: a pose at standstill takes theta of the last pose before it that defines its own -- a scan over the
        // lanes for "the last flagged value" (the operator (a, b) -> b.flag ? b : a is associative), six shuffles; lanes without a
        // flagged pose before them in this chunk take what the chunks before left.
        double cv = thcl_m + th_r;
        int cf = stand ? 0 : 1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double tv = __shfl_up(cv, o);
            const int tf = __shfl_up(cf, o);
            if (lane >= o && !cf) { cv = tv; cf = tf; }
        }
        const double th = cf ? cv : keep;
        const double thcl = stand ? th - th_r : thcl_m;
        double sn, cs;
        rp_sincos(thcl, &sn, &cs);
        const double tn = sn / cs;
        const double q = 1.0 - kr * d, cq = cs / q;
        const double kp = (dpp + (kr * dp + krd * d) * tn) * cs * (cq * cq) + cq * kr;
        const double v = sd * (q / cs);
        const double a = sdd * q / cs + ((sd * sd) / cs) * (q * tn * (kp * q / cs - kr) - (krd * d + kr * dp));
        // the step before: the neighbour lane's, lane 0 takes the last chunk's
        double th_p = __shfl_up(th, 1), kp_p = __shfl_up(kp, 1);
        if (lane == 0) { th_p = th_last; kp_p = kp_last; }
        const bool first = i == 0;
        const uint32_t code = step_reason(kin, first, v, a, kp, kp_p, th, th_p);
        const bool in_d = fabs(d) <= tb.d_limit;
        if (have && !before) {
            const uint32_t key = off ? ((uint32_t)i << 3) | RP_REASON_OUT_OF_DOMAIN
                                 : code ? ((uint32_t)i << 3) | code
                                 : !in_d ? LF_KEY_LATE | ((uint32_t)i << 3) | RP_REASON_OUT_OF_DOMAIN : LF_KEY_NONE;
            best = key < best ? key : best;
        }
        if (i < n) {
            const bool gone = !have || before || off;
            const double tx = row(seg, R_TX) + lam * row(seg, R_DTX), ty = row(seg, R_TY) + lam * row(seg, R_DTY), tl = sqrt(tx * tx + ty * ty);
            const double px = row(seg, R_PX) + lam * row(seg, R_EX), py = row(seg, R_PY) + lam * row(seg, R_EY);
            LF_PUT_POSE(i, gone || !in_d ? nan : px - d * (ty / tl), gone || !in_d ? nan : py + d * (tx / tl), gone ? nan : th, gone ? nan : v,
                        gone ? nan : a, gone ? nan : kp, gone ? nan : (first ? 0.0 : kp - kp_p), gone ? nan : thcl, !gone, s, d);
        }
        keep = __shfl(th, 63);
        th_last = keep;
        kp_last = __shfl(kp, 63);
        dead = offs != 0;
    }
