"""Tier 3 of the kinematic thresholds (tests/_kin.py): the planner's kernels (``constraint_reason`` in csrc/rp_kernels.h, through rp_plan).

Their checked quantities are computed on the device, so the DATA cannot be placed; the VEHICLE LIMIT is.  State rows do not depend on
a_max, v_switch, delta_max or v_delta_max, so the extended-precision rows of ``_xref.reference(name)`` stay the truth under any of them.
For one candidate of a case and one check: per step the value of the limit at which that step flips (acceleration: |a_i|, above
v_switch a_i v_i / v_switch; kappa: atan(wheelbase |kappa_i|) as delta_max; kappa_dot: |kd_i| wheelbase / (1 + wk^2) as v_delta_max;
yaw rate: atan(wheelbase |r_i| / (1e5 v_i)) as delta_max, under the mask without the kappa check, which reads the same limit); the
largest binds; the limit is set to it times (1 +- delta); the whole verdict is evaluated by ``_kin.exact`` on the rows under the
changed vehicle, with the production pre-filter (|s_ddot| > a_max, s_dot < -1e-5: label none) restated here.
delta_small = 64 times what the _xref rule allows the device on the rows involved (8 E_O + 8 spacings), propagated through the check
(twice over dt for the rates, times v for the product form), relative to the binding value; delta_large = 1e-6 scale.
A case is admitted only if the placed margin keeps 8 B and every other margin of every checked step -- the runner-up step, every
other check, the pre-filter -- keeps 1e-6 scale, and for the yaw rate yaw * 1e5 stays 1e-3 from a half-integer at every step:
candidates are searched on the CPU until all four versions (two deltas, two signs) of a check are admitted in both modes.
Checks run on the steps below a candidate's own length only (the reference's loop): a deciding step cannot lie in the horizon
extension, whose rows are copies."""
import functools
from types import SimpleNamespace as NS

import numpy as np

import _kin as K
import _xref as X
from _paths import LAUNCH_PATHS   # noqa: F401  (the nine launch paths the GPU test runs every case on)
from commonroad_rp_amd._capi import PlanInputs, copy_params, FLAG_DRAW_ALL, FLAG_MATERIALIZE_ALL

LD = np.longdouble
CASES = ("straight_keep_n16", "arc_keep_n17", "scurve_stop_n64", "arc_low_n65", "straight_fast_n111")   # straight, arc, S-curve, low velocity, off the block edges
LIMIT = {"acceleration": "a_max", "kappa": "delta_max", "kappa_dot": "v_delta_max", "yaw_rate": "delta_max"}
MASK = {"acceleration": 31, "kappa": 31, "kappa_dot": 31, "yaw_rate": 31 & ~K.BIT["kappa"]}
HALF_KEPT = 1e-3


LIFT_CASES = ("arc_keep_n17", "scurve_keep_n111", "scurve_stop_n64")   # the 25 m arc, the S-curve moving, and one that comes to a standstill
LIFT = "lift:"   # a case name with this prefix: the rows the LIFT has to compute from the double planes (tier 2, derived quantities)


def bare(name):
    return name[len(LIFT):] if name.startswith(LIFT) else name


@functools.lru_cache(maxsize=None)
def lift_planes(name):
    """s, s', s'', d, d', d'' [m, n] of the case's subset, the reference's rows rounded to doubles and zero behind each length, and the lengths"""
    r = X.reference(name)
    n = r.states.shape[2]
    tl = np.minimum(r.traj_len, n).astype(np.int32)
    valid = np.arange(n)[None, :] < tl[:, None]
    planes = tuple(np.where(valid, r.states[:, row, :].astype(np.float64), 0.0) for row in (X.S, X.S_DOT, X.S_DDOT, X.D, X.D_DOT, X.D_DDOT))
    return planes, tl


@functools.lru_cache(maxsize=None)
def _states(name):
    """[m, 14, n] longdouble: the planner's rows of the case, or ("lift:" + case) the lift's formulas evaluated in double-word
    arithmetic on the double planes it is given"""
    if not name.startswith(LIFT):
        return X.reference(name).states
    planes, tl = lift_planes(bare(name))
    return X.evaluate_planes(X.case(bare(name)), planes, tl)[0]


def _rows(name, j):
    r = X.reference(bare(name))
    n = r.states.shape[2]
    tl = int(min(r.traj_len[j], n))
    st = _states(name)[j]
    return NS(v=st[X.V, :tl], a=st[X.A, :tl], kappa=st[X.KAPPA, :tl], theta=st[X.THETA, :tl], s_dot=st[X.S_DOT, :tl], s_ddot=st[X.S_DDOT, :tl], tl=tl)


def vehicle(name, **changed):
    veh = K._vehicle(X.case(bare(name)).inp.params)
    for k, val in changed.items():
        setattr(veh, k, float(val))
    return veh


@functools.lru_cache(maxsize=None)
def allowance(name):
    """[14] what the _xref rule allows the device per row of this case: 8 E_O + 8 spacings of the row's scale"""
    r, status, cost, states, coeffs, mask = X.case_views(bare(name))
    sel = mask & ~X.left_out(r.states, states, mask)[:, None]
    e_o, _ = X._errors(r.states, states, sel)
    scale = np.where(sel[:, None, :], np.abs(r.states), LD(0)).max(axis=(0, 2)).astype(np.float64)
    return 8.0 * e_o + 8.0 * np.spacing(scale)


def flips(name, j, check):
    """(value of the limit at which each step flips [tl] longdouble, the binding step)"""
    q, veh = _rows(name, j), vehicle(name)
    wb, dt = LD(veh.wheelbase), LD(veh.dt)
    if check == "acceleration":
        f = np.where(q.a < 0, -q.a, np.where(q.v > LD(veh.v_switch), q.a * q.v / LD(veh.v_switch), q.a))
    elif check == "kappa":
        f = np.arctan(wb * np.abs(q.kappa))
    elif check == "kappa_dot":
        kd = np.concatenate(([LD(0)], np.diff(q.kappa))) / dt
        f = np.abs(kd) * wb / (1 + (wb * q.kappa) ** 2)
    else:
        r = np.abs(K.exact(veh, q.v, q.a, q.kappa, q.theta).r[0]).astype(LD)
        f = np.where(q.v > 0, np.arctan(wb * r / LD(100000.0) / np.where(q.v > 0, q.v, 1)), LD(0))
    return f, int(np.argmax(f))


def deltas(name, j, check):
    """(delta_small, delta_large), both relative to the binding value of the limit"""
    q, veh, al = _rows(name, j), vehicle(name), allowance(name)
    f, b = flips(name, j, check)
    if check == "acceleration":
        rel = al[X.A] / abs(float(q.a[b])) + (al[X.V] / float(q.v[b]) if q.v[b] > veh.v_switch else 0.0)
    elif check == "kappa":
        rel = al[X.KAPPA] / abs(float(q.kappa[b]))
    elif check == "kappa_dot":
        kd = abs(float(q.kappa[b] - q.kappa[b - 1])) / veh.dt
        rel = 2.0 * al[X.KAPPA] / veh.dt / kd + 2.0 * al[X.KAPPA] * veh.wheelbase
    else:
        assert 2.0 * al[X.THETA] / veh.dt * 1e5 < HALF_KEPT      # the device's yaw * 1e5 rounds to the reference's r
        rel = al[X.V] / float(q.v[b])
    ex = K.exact(vehicle(name, **{LIMIT[check]: float(f[b])}), q.v, q.a, q.kappa, q.theta)
    bound_scale = float(ex.scale[check][0, b])
    value = {"acceleration": abs(float(q.a[b])), "kappa": abs(float(q.kappa[b])), "kappa_dot": abs(float(q.kappa[b] - q.kappa[b - 1])) / veh.dt,
             "yaw_rate": float(abs(ex.r[0, b])) / 1e5}[check]
    small = max(64.0 * rel, 64.0 * K.BAND * K.U * bound_scale / value)
    return small, K.OTHER * bound_scale / value


def expected(name, j, veh, mask, draw):
    """(status word of the candidate, margins that are too small [(step, check, |g|, needed)] apart from ``placed``) -- see admitted()"""
    q = _rows(name, j)
    ex = K.exact(veh, q.v, q.a, q.kappa, q.theta)
    st = int(K.status_words(ex.fail, np.array([q.tl]), mask)[0])
    pre = []
    if not draw:   # reactive_planner.py:796-805: label stays None
        g_acc = LD(veh.a_max) - np.abs(q.s_ddot)
        g_vel = q.s_dot + LD(1e-5)
        pre = [("pre_acceleration", g_acc, veh.a_max + np.abs(q.s_ddot).astype(float)), ("pre_velocity", g_vel, np.abs(q.s_dot).astype(float) + 1e-5)]
        if (g_acc < 0).any():
            st = 0 | (K.REASON["acceleration"] << 4)
        elif (g_vel < 0).any():
            st = 0 | (K.REASON["velocity"] << 4)
    return st, ex, pre


def admitted(name, j, veh, mask, draw, placed):
    """[] if the case meets the conditions of a case, else what does not"""
    st, ex, pre = expected(name, j, veh, mask, draw)
    veh_rows = _rows(name, j)
    bad = []
    for c in K.CHECKS:
        if not mask & K.BIT[c]:
            continue
        g, sc = np.abs(ex.g[c][0]).astype(float), ex.scale[c][0]
        for i in range(len(g)):
            need = K.DECIDED * K.BAND * K.U * sc[i] if (i, c) == placed else K.OTHER * sc[i]
            if c == "yaw_rate" and (i, c) != placed and ex.yaw_firm[0, i]:
                continue
            if c == "yaw_rate" and g[i] == 0.0 and float(veh_rows.v[i]) == 0.0 and (i == 0 or veh_rows.theta[i] == veh_rows.theta[i - 1]):
                continue   # a standstill: the speed is a product with an exact zero, the orientation a copy -- 0 > 0 involves no rounding
            if not g[i] >= need:
                bad.append((i, c, g[i], need))
    if mask & K.BIT["yaw_rate"]:
        half = ex.half[0].astype(float) * 1e5
        bad += [(i, "yaw_half", half[i], HALF_KEPT) for i in range(1, len(half)) if not half[i] >= HALF_KEPT]
    for what, g, sc in pre:
        g = np.abs(g).astype(float)
        bad += [(i, what, g[i], K.OTHER * sc[i]) for i in range(len(g)) if not g[i] >= K.OTHER * sc[i]]
    return bad


@functools.lru_cache(maxsize=None)
def cases(name):
    """[namespace(check, j, index, step, sign, level, delta, limit, value, mask, want={draw: status})]: for every check the first candidate of
    the case's subset that production mode costs for which all four versions are admitted in both modes"""
    r, status, cost, states, coeffs, mask_ = X.case_views(bare(name))
    ok = ((status & 3) == 1) & X.production_feasible(bare(name)) & ~X.left_out(r.states, states, mask_)
    out = []
    # Per check: walk the candidates until one yields all four versions.  A version is given up (inner break, then the next candidate) when
    # it is not admitted in either mode, when its draw-mode word is not the intended one (feasible for "+", this check at the binding
    # step for "-"), or -- acceleration, first pass only -- when the production pre-filter stops the loosened version.
    for check in LIMIT:
        # (acceleration: first a candidate whose loosened version the production pre-filter lets through, if the case has one)
        for strict, j in [(st_, int(j_)) for st_ in ((True, False) if check == "acceleration" else (False,)) for j_ in np.flatnonzero(ok)]:
            f, b = flips(name, j, check)
            if not f[b] > 0 or (check in ("kappa_dot", "yaw_rate") and b == 0):
                continue
            small, large = deltas(name, j, check)
            made = []
            for level, delta in (("small", small), ("large", large)):
                for sign in (+1, -1):
                    value = float(f[b] * (1 + LD(sign * delta)))
                    veh = vehicle(name, **{LIMIT[check]: value})
                    if any(admitted(name, j, veh, MASK[check], draw, (b, check)) for draw in (False, True)):
                        break
                    want = {draw: expected(name, j, veh, MASK[check], draw)[0] for draw in (False, True)}
                    if want[True] != (1 if sign > 0 else 2 | (K.REASON[check] << 4) | (b << 8)):
                        break
                    if strict and sign > 0 and want[False] != 1:
                        break
                    made.append(NS(check=check, j=j, index=int(r.index[j]), step=b, sign=sign, level=level, delta=delta, limit=LIMIT[check], value=value,
                                   mask=MASK[check], want=want, tl=_rows(name, j).tl))
                else:
                    continue
                break
            if len(made) == 4:
                out += made
                break
    # two checks and more failing in one step: delta_max and v_delta_max at half of what step 1 needs, under the full mask and without
    # the kappa check (nothing is placed: every margin keeps 1e-6 scale)
    for j in np.flatnonzero(ok):
        j = int(j)
        fk, fd = flips(name, j, "kappa")[0], flips(name, j, "kappa_dot")[0]
        if len(fk) < 3 or not (fk[1] > 0 and fd[1] > 0):
            continue
        veh = vehicle(name, delta_max=float(fk[1]) / 2, v_delta_max=float(fd[1]) / 2)
        made = []
        for mask in (31, 31 & ~K.BIT["kappa"]):
            if any(admitted(name, j, veh, mask, draw, None) for draw in (False, True)):
                break
            made.append(NS(check="priority", j=j, index=int(r.index[j]), step=1, sign=-1, level="half", delta=0.5, limit="delta_max", value=veh.delta_max,
                           also=("v_delta_max", veh.v_delta_max), mask=mask, want={draw: expected(name, j, veh, mask, draw)[0] for draw in (False, True)},
                           tl=_rows(name, j).tl))
        if len(made) == 2:
            out += made
            break
    return out


def plan_inputs(name, c, draw):
    inp = X.case(bare(name)).inp
    p = copy_params(inp.params)
    setattr(p, c.limit, c.value)
    if getattr(c, "also", None):
        setattr(p, *c.also)
    p.constraint_mask = c.mask
    p.flags = (p.flags & ~(FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)) | (FLAG_DRAW_ALL if draw else 0)
    return PlanInputs(p, inp.cost, inp.T, inp.traj_len, inp.L, inp.D)


def lift_call(name, c):
    """(params, keyword arguments) of the lift call of a case version: every candidate of the subset as a trajectory"""
    inp = plan_inputs(name, c, True)
    planes, tl = lift_planes(name)
    return inp.params, dict(zip(("s", "s_dot", "s_ddot", "d", "d_dot", "d_ddot"), planes), lengths=tl)


def summary_lines():
    lines = ["tier 3, the planner's kernels (rp_plan): per case and check the candidate, its binding step / own length, delta_small and delta_large",
             "(relative to the limit's binding value), expected status words (production, draw) of the four versions"]
    for name in CASES + tuple(LIFT + q for q in LIFT_CASES):
        if name == LIFT + LIFT_CASES[0]:
            lines += ["", "tier 2, derived quantities (rp_lift_evaluate on the double planes of the same candidates; the draw-mode word is the lift's):"]
        for c in cases(name):
            if c.check == "priority":
                lines.append(f"  {name:20s} priority     candidate {c.index:4d} delta_max = {c.value:.6g} {c.also[0]} = {c.also[1]:.6g} mask {c.mask:2d}  "
                             f"want {c.want[False]:#x}/{c.want[True]:#x}")
            if c.level == "small" and c.sign > 0:
                d = {(q.level, q.sign): q for q in cases(name) if q.check == c.check}
                lines.append(f"  {name:20s} {c.check:12s} candidate {c.index:4d} step {c.step:3d} / {c.tl:3d}  {c.limit} = {c.value:.6g}  delta_small {d['small', 1].delta:.2e} "
                             f"delta_large {d['large', 1].delta:.2e}  want " + " ".join(f"{q.want[False]:#x}/{q.want[True]:#x}" for q in d.values()))
        missing = sorted((set(LIMIT) | {"priority"}) - {c.check for c in cases(name)})
        if missing:
            lines.append(f"  {name:20s} no candidate admitted for: {', '.join(missing)}")
    return lines + [""] + velocity_lines()


def device_lines():
    """per case and launch path (tier 3), per case (tier 2): plans or calls made / verdicts that differ from the reference's"""
    from commonroad_rp_amd._capi import RpContext
    from commonroad_rp_amd.collision import ObstacleTables
    from commonroad_rp_amd.lift import TrajectoryLifter
    lines = ["device verdicts of tier 3 (per case: launch path differ/plans, production and draw mode):"]
    for name in CASES:
        found = []
        for path, opts in LAUNCH_PATHS.items():
            ctx = RpContext(0)
            try:
                for k, v in opts.items():
                    ctx.set_option(k, v)
                ctx.set_coordinate_system(X.case(name).co)
                ctx.set_obstacles(ObstacleTables())
                differ = plans = 0
                for c in cases(name):
                    for draw in (False, True):
                        ctx.plan(plan_inputs(name, c, draw))
                        plans += 1
                        differ += int(ctx.fetch_status()[0][c.index]) != int(c.want[draw])
                found.append(f"{path} {differ}/{plans}")
            finally:
                ctx.close()
        lines.append(f"  {name:20s} " + "  ".join(found))
    lines.append("device verdicts of the velocity cases (per case: launch path differ/status words, two masks x two modes):")
    for name in VELOCITY_CASES:
        found = []
        for path, opts in LAUNCH_PATHS.items():
            ctx = RpContext(0)
            try:
                for k, v in opts.items():
                    ctx.set_option(k, v)
                ctx.set_coordinate_system(X.case(name).co)
                ctx.set_obstacles(ObstacleTables())
                differ = total = 0
                for mask in VELOCITY_MASKS:
                    for draw in (False, True):
                        ctx.plan_coeffs(*velocity_plan(name, mask, draw))
                        got, want = ctx.fetch_status()[0], velocity_cases(name).want[mask, draw]
                        differ, total = differ + int((got != want).sum()), total + len(want)
                found.append(f"{path} {differ}/{total}")
            finally:
                ctx.close()
        lines.append(f"  {name:20s} " + "  ".join(found))
    lines.append("device verdicts of tier 2, derived quantities (differ/calls):")
    for name in LIFT_CASES:
        with TrajectoryLifter(0) as lf:
            lf.set_reference(X.case(name).co)
            differ = 0
            for c in cases(LIFT + name):
                p, kw = lift_call(name, c)
                differ += int(lf.lift(p, **kw).status[c.j]) != int(c.want[True])
        lines.append(f"  {name:20s} {differ}/{len(cases(LIFT + name))}")
    return lines


# ---- the velocity check: no limit to place, so the polynomial is (rp_plan_coeffs, explicit polynomials on a straight path) -----------
# s_dot(t) = m + k (t - t_m)^2 with its minimum m on the grid step i_m; d constant.  On a straight path with d_dot = 0 the speed v IS
# s_dot, and the reference's rule |s_dot| < 1e-5 -> 0 stands in front of the check: with min s_dot above -1e-5 the pose is a standstill
# (v = 0, orientation kept, feasible), below it v < -1e-5 fails the velocity check at that step (production: the pre-filter
# s_dot < -1e-5, label none).  The coefficient c1 is adjusted IN THE REFERENCE (s_dot of the double coefficients in double-word
# arithmetic, two correction steps: what a bisection converges to) until the minimum sits at -1e-5 +- delta.
# On the 25 m arc at d = 2 m the speed is v = s_dot (1 - k_r d) = 0.92 s_dot: there the minimum of V is placed at -1e-5 +- delta, with s_dot
# at -1.09e-5 clear of its own rule -- the one place where the planner's v lies between -1e-5 and 0 ("v < 0" would fail it).  The pose
# is a standstill with v < 0, so under the full mask the yaw-rate check (0 > kappa_max v) fails where the velocity check passes, and
# in production the pre-filter stops all four versions: the velocity check alone in draw mode is where "+" is feasible.
VELOCITY_CASES = {"straight_keep_n16": (5, 1.0), "straight_fast_n111": (96, 0.05), "arc_keep_n17": (5, 1.0)}   # case -> (i_m, k): lanes 5, 0 (block 6), 5
VELOCITY_MASKS = (31, K.BIT["velocity"])
S0 = 12.3


def _lon(c1, k, t_m):
    return np.array([S0, c1, -k * t_m, k / 3.0, 0.0, 0.0])


def raw_s_dot(lon, n, dt):
    """s_dot of the double coefficients at the n grid steps, before the reference's 1e-5 rule: double-word, rounded to longdouble"""
    t = K.DD(np.arange(n).astype(LD)) * K.DD(LD(dt))
    cl = [K.DD(np.full(n, LD(q))) for q in lon]
    t2 = t * t
    return X._vel(cl, t, t2, t2 * t, t2 * t2).ld()


@functools.lru_cache(maxsize=None)
def velocity_cases(name):
    """namespace(lon [4, 6], lat [4, 6], T [4], tl [4], versions [(level, sign, delta, g)], step, want={(mask, draw): status [4]},
    counts={(mask, draw): [8]}, e_o, B): the four versions of a case as the four candidates of one rp_plan_coeffs call"""
    from oracle import oracle
    c = X.case(name)
    p = c.inp.params
    n, dt = p.N + 1, float(p.dt)
    i_m, k = VELOCITY_CASES[name]
    t_m = i_m * dt
    lat = np.array([float(p.x0_lat[0]), 0.0, 0.0, 0.0, 0.0, 0.0])
    eps = LD(1e-5)

    on_v = not name.startswith("straight")                  # the placed quantity: the row V where it is not s_dot itself
    one = np.array([n], dtype=np.int32)

    def v_min(lon):
        return X.evaluate(c, lon[None].astype(LD), lat[None].astype(LD), one)[0][0, X.V, i_m]

    probe = _lon(k * t_m * t_m - 2e-5, k, t_m)             # s_dot = -2e-5 at the minimum, clear of the 1e-5 rule: v / s_dot there
    factor = v_min(probe) / raw_s_dot(probe, n, dt)[i_m] if on_v else LD(1)

    def place(target):
        c1 = float(LD(k * t_m * t_m) + target / factor)
        for _ in range(3):
            lon = _lon(c1, k, t_m)
            c1 = float(LD(c1) + ((target - v_min(lon)) / factor if on_v else target - raw_s_dot(lon, n, dt)[i_m]))
        return _lon(c1, k, t_m)
    # what the _xref rule allows the device on the s_dot row of these polynomials: 8 E_O + 8 spacings of the row's scale
    nominal = place(-2 * eps)                                # (clear of the 1e-5 rule: the oracle and the reference take the same branch)
    run = oracle.plan_coeffs(X.with_flags(c.inp, set_=FLAG_DRAW_ALL).params, c.inp.cost, c.tables, nominal[None], lat[None], np.array([n], dtype=np.int32))
    raw = raw_s_dot(nominal, n, dt)
    ref_row = X.evaluate(c, nominal[None].astype(LD), lat[None].astype(LD), one)[0][0, X.V]
    e_o = float(np.abs(run.states[0, X.V].astype(LD) - ref_row).max())
    terms = abs(nominal[1]) + 2 * abs(nominal[2]) * (n - 1) * dt + 3 * abs(nominal[3]) * ((n - 1) * dt) ** 2 + 1e-5
    B = K.BAND * K.U * terms
    small = 64.0 * (8.0 * e_o + 8.0 * float(np.spacing(np.abs(raw).max().astype(np.float64))))
    large = K.OTHER * 2e-5                                  # 1e-6 of the bound's own scale, |v| + 1e-5
    versions, lons = [], []
    for level, delta in (("small", small), ("large", large)):
        for sign in (+1, -1):
            lon = place(-eps + LD(sign * delta))
            g = float((v_min(lon) if on_v else raw_s_dot(lon, n, dt)[i_m]) + eps)
            versions.append((level, sign, delta, g))
            lons.append(lon)
    lon, lat4 = np.stack(lons), np.tile(lat, (4, 1))
    tl = np.full(4, n, dtype=np.int32)
    rows = X.evaluate(c, lon.astype(LD), lat4.astype(LD), tl)[0]
    veh = vehicle(name)
    ex = K.exact(veh, rows[:, X.V], rows[:, X.A], rows[:, X.KAPPA], rows[:, X.THETA])
    want, counts = {}, {}
    for mask in VELOCITY_MASKS:
        for draw in (False, True):
            st = K.status_words(ex.fail, tl, mask).astype(np.int64)
            if not draw:                                    # the pre-filter (reactive_planner.py:796-805) runs after the 1e-5 rule
                st = np.where((rows[:, X.S_DOT] < -eps).any(axis=1), 0 | (K.REASON["velocity"] << 4), st)
            want[mask, draw] = st.astype(np.uint32)
            counts[mask, draw] = np.bincount((st[st != 1] >> 4) & 7, minlength=8)
    return NS(name=name, lon=lon, lat=lat4, T=np.full(4, (n - 1) * dt), tl=tl, versions=versions, step=i_m, want=want, counts=counts, e_o=e_o, B=B,
              small=small, large=large, rows=rows, exact=ex, veh=veh, on_v=on_v, raw=np.stack([raw_s_dot(q, n, dt) for q in lons]))


def velocity_not_admitted(v):
    """[] if the four versions meet the conditions of a case: the placed margin s_dot + 1e-5 at the minimum has the intended sign and keeps
    8 B; every other step keeps 1e-6 scale from +-1e-5 and from 0.001; every other check keeps 1e-6 scale, where the yaw rate of an
    orientation that is kept (a copy: an exact 0) is measured against kappa_max |v| alone and 0 > 0 is left out"""
    bad = []
    kmax = float(K.kappa_max_dd(v.veh).ld())
    for q, (level, sign, delta, g) in enumerate(v.versions):
        if not (np.sign(g) == sign and abs(g) >= K.DECIDED * v.B and 0.5 * delta <= abs(g) <= 2.0 * delta):
            bad.append((q, "placed", g, delta))
        raw = v.raw[q].astype(np.float64)
        for i in range(len(raw)):
            if (i != v.step or v.on_v) and not (abs(abs(raw[i]) - 1e-5) >= K.OTHER * (abs(raw[i]) + 1e-5) and abs(raw[i] - 0.001) >= K.OTHER * (abs(raw[i]) + 0.001)):
                bad.append((q, "s_dot rules", i, raw[i]))
        theta = v.rows[q, X.THETA]
        for c in K.CHECKS:
            g_c, sc = np.abs(v.exact.g[c][q]).astype(float), v.exact.scale[c][q].copy()
            for i in range(len(g_c)):
                if c == "velocity" and i == v.step:
                    continue                                # (the placed one; on a straight path "+" is behind the 1e-5 rule: v = 0)
                if c == "yaw_rate" and i > 0 and theta[i] == theta[i - 1]:
                    if g_c[i] == 0.0:
                        continue
                    sc[i] = kmax * abs(float(v.rows[q, X.V, i]))
                elif c == "yaw_rate" and i > 0 and not float(v.exact.half[q, i]) * 1e5 >= HALF_KEPT:
                    bad.append((q, "yaw_half", i, float(v.exact.half[q, i])))
                if not g_c[i] >= K.OTHER * sc[i]:
                    bad.append((q, c, i, g_c[i], K.OTHER * sc[i]))
    return bad


def velocity_plan(name, mask, draw):
    """(params, cost, lon, lat, T, traj_len) of the rp_plan_coeffs call"""
    v, inp = velocity_cases(name), X.case(name).inp
    p = copy_params(inp.params)
    p.constraint_mask = mask
    p.flags = (p.flags & ~(FLAG_DRAW_ALL | FLAG_MATERIALIZE_ALL)) | (FLAG_DRAW_ALL if draw else 0)
    return p, inp.cost, v.lon, v.lat, v.T, v.tl


def velocity_lines():
    lines = ["tier 3, the velocity check (rp_plan_coeffs, s_dot = m + k (t - t_m)^2, d constant; min v at -1e-5 +- delta; absolute, m/s):"]
    for name in VELOCITY_CASES:
        v = velocity_cases(name)
        lines.append(f"  {name:20s} step {v.step:3d}  B {v.B:.2e}  E_O {v.e_o:.2e}  delta_small {v.small:.2e} delta_large {v.large:.2e}  placed v + 1e-5: "
                     + " ".join(f"{g:+.3e}" for _, _, _, g in v.versions) + "  want (full mask: production / draw) "
                     + " ".join(f"{a:#x}/{b:#x}" for a, b in zip(v.want[31, False], v.want[31, True])))
    return lines
