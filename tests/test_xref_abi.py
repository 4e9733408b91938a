"""What tests/test_xref.py (GPU) rests on, checked without a GPU: the extended-precision reference of tests/_xref.py against an mpmath
evaluation at 50 digits, the double oracle and oracle/numpy_loop.py against the reference (E_O <= 1e-11 per case and row; measured: a few
1e-12 at most, printed below), the cap on the candidates left out of the comparison, and the sensitivity of the comparison itself --
planted defects of the eighth-digit-and-beyond kind must fail it, the oracle itself and numpy_loop's rows must pass it."""
import functools
import math

import numpy as np
import pytest

import _xref as XR

pytestmark = pytest.mark.skipif(not XR.HAVE_LONGDOUBLE, reason=XR.SKIP_REASON)
LD = XR.LD


# ---- the reference against mpmath ----------------------------------------------------------------------------------------------------
MP_CASES = ("arc_low_n65", "scurve_stop_n64", "straight_still0_n65")


def _mp_candidate(mp, c, index):
    """oracle/numpy_loop.py's sample + evaluate for ONE candidate, straight-line, in mpmath numbers (no feasibility decisions):
    -> (rows [14][n], cost)"""
    F = mp.mpf
    p, tb, cst, inp = c.inp.params, c.tables, c.inp.cost, c.inp
    n, dt = p.N + 1, F(p.dt)
    eps, two_pi, pi = F(1e-5), F(2.0 * math.pi), F(math.pi)

    def solve(a, b):
        return list(mp.lu_solve(mp.matrix(a), mp.matrix(b)))

    def quintic(x0, xd, T):
        t2 = T * T
        t3, t4 = t2 * T, t2 * t2
        t5 = t4 * T
        h = solve([[t3, t4, t5], [3 * t2, 4 * t3, 5 * t4], [6 * T, 12 * t2, 20 * t3]],
                  [xd[0] - (x0[0] + x0[1] * T + F(0.5) * x0[2] * t2), xd[1] - (x0[1] + x0[2] * T), xd[2] - x0[2]])
        return [x0[0], x0[1], F(0.5) * x0[2], h[0], h[1], h[2]]

    def quartic(x0, vd, T):
        t2 = T * T
        t3 = t2 * T
        h = solve([[3 * t2, 4 * t3], [6 * T, 12 * t2]], [vd - x0[1] - x0[2] * T, -x0[2]])
        return [x0[0], x0[1], F(0.5) * x0[2], h[0], h[1], F(0)]

    pos = lambda k, t: k[0] + k[1] * t + k[2] * t ** 2 + k[3] * t ** 3 + k[4] * t ** 4 + k[5] * t ** 5
    vel = lambda k, t: k[1] + 2 * k[2] * t + 3 * k[3] * t ** 2 + 4 * k[4] * t ** 3 + 5 * k[5] * t ** 4
    acc = lambda k, t: 2 * k[2] + 6 * k[3] * t + 12 * k[4] * t ** 2 + 20 * k[5] * t ** 3

    nL, nD = len(inp.L), len(inp.D)
    iT, rem = divmod(int(index), nL * nD)
    iL, iD = divmod(rem, nD)
    T = F(float(inp.T[iT]))
    x0_lon, x0_lat = [F(v) for v in p.x0_lon], [F(v) for v in p.x0_lat]
    zero = F(0)
    lon = quintic(x0_lon, [F(float(inp.L[iL])), zero, zero], T) if p.lon_mode == 1 else quartic(x0_lon, F(float(inp.L[iL])), T)
    tau = T
    if p.low_vel_mode:
        s_goal = pos(lon, T) - x0_lon[0]
        tau = s_goal if s_goal > 0 else T
    lat = quintic(x0_lat, [F(float(inp.D[iD])), zero, zero], tau)
    L = min(int(inp.traj_len[iT]), n)

    rp, rth, rk, rkd = ([F(float(v)) for v in a] for a in (tb.ref_pos, tb.ref_theta, tb.ref_curv, tb.ref_curv_d))
    rx, ry = [F(float(v)) for v in tb.ref_x], [F(float(v)) for v in tb.ref_y]
    nr = len(rp)
    ux, uy = [], []
    for k in range(nr - 1):
        ex, ey = rx[k + 1] - rx[k], ry[k + 1] - ry[k]
        ln = mp.sqrt(ex * ex + ey * ey)
        ux.append(ex / ln); uy.append(ey / ln)
    tx, ty = [ux[0]], [uy[0]]
    for k in range(1, nr - 1):
        ax, ay = ux[k - 1] + ux[k], uy[k - 1] + uy[k]
        ln = mp.sqrt(ax * ax + ay * ay)
        tx.append(ax / ln); ty.append(ay / ln)
    tx.append(ux[-1]); ty.append(uy[-1])

    def valid_orientation(a):
        a = a % two_pi
        return a - two_pi if pi <= a <= two_pi else a

    st = [[zero] * n for _ in range(14)]
    for i in range(L):
        t = F(i) * dt
        s, sv, sa = pos(lon, t), vel(lon, t), acc(lon, t)
        if not p.low_vel_mode:
            d, dv, da = pos(lat, t), vel(lat, t), acc(lat, t)
        else:
            s1 = s - pos(lon, zero)
            d, dv, da = pos(lat, s1), vel(lat, s1), acc(lat, s1)
        if abs(sv) < eps:
            sv = zero
        if abs(dv) < eps:
            dv = zero
        moving = sv > F(0.001)
        if not p.low_vel_mode:
            dp = dv / sv if moving else zero
            dpp = (da - dp * sa) / (sv * sv) if moving else zero
        else:
            dp, dpp = dv, da
        k = sum(1 for v in rp if not v > s) - 1        # np.argmax(ref_pos > s) - 1 inside the domain
        k = min(max(k, 0), nr - 2)
        lam = (s - rp[k]) / (rp[k + 1] - rp[k])
        th_ref = valid_orientation((rth[k + 1] - rth[k]) * (s - rp[k]) / (rp[k + 1] - rp[k]) + rth[k])
        if moving or p.low_vel_mode:
            theta_cl = mp.atan2(dp, 1)
            theta = theta_cl + th_ref
        else:
            theta = F(p.x0_orientation) if i == 0 else st[XR.THETA][i - 1]
            theta_cl = theta - th_ref
        k_r = (rk[k + 1] - rk[k]) * lam + rk[k]
        k_r_d = (rkd[k + 1] - rkd[k]) * lam + rkd[k]
        one_krd = 1 - k_r * d
        cos_t, tan_t = mp.cos(theta_cl), mp.tan(theta_cl)
        kappa = (dpp + (k_r * dp + k_r_d * d) * tan_t) * cos_t * (cos_t / one_krd) ** 2 + (cos_t / one_krd) * k_r
        v = sv * (one_krd / cos_t)
        a = sa * one_krd / cos_t + ((sv * sv) / cos_t) * (one_krd * tan_t * (kappa * one_krd / cos_t - k_r) - (k_r_d * d + k_r * dp))
        px, py = rx[k] + lam * (rx[k + 1] - rx[k]), ry[k] + lam * (ry[k + 1] - ry[k])
        ax, ay = tx[k] + lam * (tx[k + 1] - tx[k]), ty[k] + lam * (ty[k + 1] - ty[k])
        tn = mp.sqrt(ax * ax + ay * ay)
        for r, val in ((XR.X, px - d * (ay / tn)), (XR.Y, py + d * (ax / tn)), (XR.THETA, theta), (XR.V, v), (XR.A, a), (XR.KAPPA, kappa),
                       (XR.S, s), (XR.D, d), (XR.THETA_CL, theta_cl), (XR.S_DOT, sv), (XR.S_DDOT, sa), (XR.D_DOT, dv), (XR.D_DDOT, da)):
            st[r][i] = val
    for i in range(1, n):
        st[XR.KAPPA_DOT][i] = st[XR.KAPPA][i] - st[XR.KAPPA][i - 1]
    if n > L:   # trajectories.py:168-197, 302-332 (oracle/numpy_loop._enlarge)
        last = L - 1
        a_last = st[XR.A][last]            # a[-1] is read after the row is extended
        s_dd_pad, d_dd_pad = st[XR.S_DDOT][n - 1], st[XR.D_DDOT][n - 1]   # ... s_ddot[-1] and d_ddot[-1] before: the zero padding
        accx = accy = zero
        for j in range(1, n - L + 1):
            t, i = F(j) * dt, last + j
            vt = st[XR.V][last] + t * a_last
            vt = vt if vt >= 0 else zero
            sd = st[XR.S_DOT][last] + t * s_dd_pad
            sd = sd if sd >= 0 else zero
            accx += dt * vt * mp.cos(st[XR.THETA][last])
            accy += dt * vt * mp.sin(st[XR.THETA][last])
            st[XR.A][i], st[XR.V][i] = a_last, vt
            for r in (XR.THETA, XR.KAPPA, XR.KAPPA_DOT, XR.S_DDOT, XR.D_DDOT, XR.THETA_CL):
                st[r][i] = st[r][last]
            st[XR.X][i], st[XR.Y][i] = st[XR.X][last] + accx, st[XR.Y][last] + accy
            st[XR.S_DOT][i], st[XR.D_DOT][i] = sd, st[XR.D_DOT][last] + t * d_dd_pad
            st[XR.S][i] = st[XR.S][last] + t * st[XR.S_DOT][last]
            st[XR.D][i] = st[XR.D][last] + t * st[XR.D_DOT][last]
    a, v, s, d, th = st[XR.A], st[XR.V], st[XR.S], st[XR.D], st[XR.THETA_CL]
    q = F(0.25)
    tail = sum((q * abs(x)) ** 2 for x in th) + (5 * abs(th[-1])) ** 2
    if cst.kind == 1:
        cost = sum(x ** 2 for x in a) + sum((q * x) ** 2 for x in d) + (20 * d[-1]) ** 2 + tail
    else:
        cost = sum((F(cst.w_a) * x) ** 2 for x in a)
        if not math.isnan(cst.desired_speed):
            vd = F(cst.desired_speed)
            cost += sum((5 * (x - vd)) ** 2 for x in v) + 50 * (v[-1] - vd) ** 2 + 100 * (v[int(n / 2)] - vd) ** 2
        if not math.isnan(cst.desired_s):
            ds = F(cst.desired_s)
            cost += sum((q * (ds - x)) ** 2 for x in s) + (20 * (ds - s[-1])) ** 2
        dd = F(cst.desired_d)
        cost += sum((q * (dd - x)) ** 2 for x in d) + (20 * (dd - d[-1])) ** 2 + tail
    return st, cost


@functools.lru_cache(maxsize=None)
def _mp_errors(name):
    """per row: (largest |reference - 50-digit evaluation| over 3 feasible candidates (first, middle, last), the rows' scale there);
    the same for the cost, relative"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    c = XR.case(name)
    ref, status, *_ = XR.case_views(name)
    feas = np.flatnonzero((status & 3) == 1)
    err, scale, cost_err = [mp.mpf(0)] * 14, [mp.mpf(0)] * 14, mp.mpf(0)
    for j in (feas[0], feas[len(feas) // 2], feas[-1]):
        st, cost = _mp_candidate(mp, c, ref.index[j])
        for r in range(14):
            scale[r] = max(scale[r], max(abs(v) for v in st[r]))
            err[r] = max(err[r], max(abs(_mpf(mp, ref.states[j, r, i]) - st[r][i]) for i in range(len(st[r]))))
        cost_err = max(cost_err, abs(_mpf(mp, ref.cost[j]) - cost) / cost)
    return err, scale, cost_err


@pytest.mark.parametrize("name", MP_CASES)
def test_reference_matches_mpmath(name, capsys):
    """Every row of the reference within 16 * 2^-64 of the 50-digit evaluation, relative to the row's scale (scale[r] of the case:
    tests/_xref.py).  Measured: below 1 unit on every row -- the rows are worked out in double-word longdouble arithmetic (tests/_dd.py)
    and handed out rounded.  (In plain longdouble the rows that are differences of nearly equal numbers miss this bound: kappa_dot,
    np.diff of kappa, by 50 .. 1e5 units; theta - theta_ref from a standstill on a straight path is a rounding residue altogether.)"""
    pytest.importorskip("mpmath")
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    scale = [r.scale for r in XR.compare_rows(ref.states, states, states, mask)[0]]
    err, _, cost_err = _mp_errors(name)
    unit = 2.0 ** -64
    with capsys.disabled():
        print(f"\n{name}: |reference - mpmath| in units of 2^-64 x scale: " +
              " ".join(f"{XR.ROWS[r]}={float(err[r]) / (unit * scale[r]) if scale[r] else 0.0:.3g}" for r in range(14)) +
              f" cost={float(cost_err / unit):.3g}")
    bad = [XR.ROWS[r] for r in range(14) if not float(err[r]) <= 16 * unit * scale[r]]
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", MP_CASES)
def test_reference_is_far_closer_to_mpmath_than_the_bounds_it_serves(name):
    """What the device tests need of the reference: its own distance to the 50-digit evaluation is at most 2^-8 of the bound a device row
    is held to in that case (8 E_O + 8 spacing(scale)), so that it moves no verdict; costs: 2^-8 of the summation bound."""
    pytest.importorskip("mpmath")
    c = XR.case(name)
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    rows, _ = XR.compare_rows(ref.states, states, states, mask)
    err, scale, cost_err = _mp_errors(name)
    bad = [(r.row, float(err[k]), r.e_bound) for k, r in enumerate(rows) if not float(err[k]) <= r.e_bound / 256]
    assert not bad, (name, bad)
    assert float(cost_err) <= XR.summation_bound(c.inp.params.N) / 256


def _mpf(mp, x):
    """a longdouble as an mpmath number, exactly: high double + remainder"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


# ---- the oracles against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", XR.CASE_NAMES)
def test_oracle_within_1e11_of_the_reference_and_nothing_left_out(name, capsys):
    c = XR.case(name)
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    assert len(ref.index) <= XR.MAX_EVALUATED and c.inp.n_candidates <= 600
    assert mask.any(axis=1).all()      # every evaluated candidate is compared on something
    rows, n_out = XR.compare_rows(ref.states, states, states, mask)
    with capsys.disabled():
        print(f"\n{name}: {len(ref.index)} of {c.inp.n_candidates} candidates evaluated, {n_out} left out")
        for r in rows:
            print(f"  {r.row:>9s} scale {r.scale:9.3e}  E_O {r.e_o:9.3e}  R_O {r.r_o:9.3e}")
    # the cap on what the comparison leaves out: nothing, except in the cases named as degenerate (2 % of the evaluated candidates)
    assert n_out <= (0.02 * len(ref.index) if c.spec.degenerate else 0), (name, n_out)
    assert max(r.e_o for r in rows) <= XR.ORACLE_BOUND, [r.line() for r in rows if r.e_o > XR.ORACLE_BOUND]
    assert not XR.failures(rows)       # the oracle passes its own comparison
    sel = ((status & 3) == 1) & ~XR.left_out(ref.states, states, mask)
    e_o, _, bound = XR.compare_costs(ref.cost, cost, cost, sel, c.inp.params.N)
    assert e_o <= 1e-11 and e_o <= bound
    e_c, _, ok = XR.compare_coeffs(np.concatenate((ref.lon, ref.lat), axis=1), coeffs[:, :12], coeffs[:, :12])
    assert ok and (e_c <= 1e-9 * np.maximum(1.0, np.abs(coeffs[:, :12]))).all()


@pytest.mark.parametrize("name", XR.CASE_NAMES)
def test_numpy_loop_within_1e11_of_the_reference(name):
    from oracle import numpy_loop as NL
    c = XR.case(name)
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    env = NL._Env(c.inp.params, c.inp.cost, c.tables)
    rows_nl = np.zeros_like(states)
    for j, i in enumerate(ref.index):
        lon, lat, tl = NL.sample(c.inp.params, c.inp, int(i))
        st_word, cst, st = NL.evaluate(env, lon, lat, tl)
        assert st is not None and (st_word & 3) == (status[j] & 3), (name, int(i), hex(st_word), hex(int(status[j])))
        rows_nl[j] = st
        if (st_word & 3) == 1:
            assert abs(LD(cst) - ref.cost[j]) <= 1e-11 * ref.cost[j]
    rows, n_out = XR.compare_rows(ref.states, states, rows_nl, mask)
    assert max(r.e_d for r in rows) <= XR.ORACLE_BOUND, [r.line() for r in rows if r.e_d > XR.ORACLE_BOUND]
    assert not XR.failures(rows), XR.failures(rows)      # numpy_loop's rows pass the comparison


def test_coefficient_tier_oracle_within_1e11():
    """the rp_plan_coeffs tier (the reference's coefficients rounded to double, evaluated by both): same labels, same bound"""
    for name in XR.CASE_NAMES:
        c = XR.case(name)
        lon, lat, T, tl, ref, status, cost, states = XR.coeffs_tier(name)
        mask = XR.compared_steps(status, c.inp.params.N + 1, c.spec.draw)
        rows, n_out = XR.compare_rows(ref.states, states, states, mask)
        assert mask.any() and n_out <= (0.02 * len(tl) if c.spec.degenerate else 0), (name, n_out)
        assert max(r.e_o for r in rows) <= XR.ORACLE_BOUND, (name, [r.line() for r in rows if r.e_o > XR.ORACLE_BOUND])


def test_cases_cover_the_shapes():
    specs = XR.CASES
    assert {s.n_steps for s in specs} == {16, 17, 64, 65, 111}
    assert {s.start for s in specs} == {"keep", "fast", "stop", "low", "still0", "still002"}
    assert {s.path for s in specs} >= {"straight_nw", "straight_se", "arc", "scurve"}
    assert {(s.cost, s.w_a) for s in specs} >= {("default", 1.0), ("default", 5.0)} and any(s.cost == "failsafe" for s in specs)
    assert {s.desired_d for s in specs} == {0.0, 0.5}
    assert sum(s.draw for s in specs) >= 2 and any(s.ragged_T for s in specs)
    for s in specs:
        c = XR.case(s.name)
        p = c.inp.params
        assert p.constraint_mask == 31 and p.flags & XR.FLAG_SKIP_COLLISION and bool(p.flags & XR.FLAG_DRAW_ALL) == s.draw
        assert c.inp.traj_len.min() == 3 and c.inp.traj_len.max() == s.n_steps       # shortest time sample 2 dt
        ref = XR.reference(s.name)
        assert ref.traj_len.min() == 3 or s.start in ("stop", "low"), s.name           # (nothing stops or turns in 2 dt)
        assert ref.traj_len.max() == s.n_steps
        d0 = c.inp.D[ref.index % len(c.inp.D)] == p.x0_lat[0]
        assert d0.any()
        if s.ragged_T:
            off = np.abs(c.inp.T / XR.DT - np.round(c.inp.T / XR.DT)) > 0.1
            assert off.any() and (c.inp.traj_len[off] * XR.DT > c.inp.T[off] + 0.05).all()   # evaluated beyond T
        if s.path.startswith("straight"):
            assert np.abs(ref.states[:, :2, 0]).min() > 480.0
        if s.path == "arc" and s.n_steps >= 64:
            assert np.abs(ref.states[:, XR.D, :]).max() >= 3.9 and abs(abs(ref.inter["k_r"][0, 0]) - 0.04) < 1e-3
        if s.start.startswith("still"):   # the carried-theta branch is on compared elements
            inside = np.arange(s.n_steps)[None, :] < ref.traj_len[:, None]
            carried = inside & (ref.states[:, XR.S_DOT, :] <= 0.001)
            assert carried.any(axis=1).sum() >= 4, s.name
            if s.start == "still0":
                assert carried[:, 0].all() and (ref.states[:, XR.THETA, 0] == LD(p.x0_orientation)).all()


# ---- sensitivity: planted defects fail the comparison ----------------------------------------------------------------------------------
SENS_CASE = "straight_stop_n65"    # a quintic on both axes, x and y near +-500


def _planted(ref_rows, states, defect_rows):
    """the oracle's rows moved by what the defect moves the reference (rounded to double)"""
    return states + (defect_rows - ref_rows).astype(np.float64)


@pytest.mark.parametrize("row", ["x", "y", "s", "v", "theta"])
def test_a_row_off_by_2_to_the_minus_40_fails(row):
    ref, status, cost, states, coeffs, mask = XR.case_views(SENS_CASE)
    bad = states.copy()
    bad[:, XR.ROWS.index(row), :] *= 1.0 + 2.0 ** -40
    rows, _ = XR.compare_rows(ref.states, states, bad, mask)
    assert [r.row for r in rows if not r.ok] == [row]


def test_one_element_of_x_off_by_64_ulp_fails():
    ref, status, cost, states, coeffs, mask = XR.case_views(SENS_CASE)
    rows, _ = XR.compare_rows(ref.states, states, states, mask)
    bad = states.copy()
    bad[3, XR.X, 7] += 64 * np.spacing(rows[XR.X].scale)
    rows, _ = XR.compare_rows(ref.states, states, bad, mask)
    assert [r.row for r in rows if not r.ok] == ["x"]


@pytest.mark.parametrize("name", ["arc_failsafe_n64", "scurve_keep_n111"])
def test_theta_cl_from_a_cosine_off_by_1e_12_fails(name):
    """theta_cl recomputed from a cosine that is off by 1e-12 relative (sign kept): it moves by 1e-12 / tan(theta_cl)"""
    ref, status, cost, states, coeffs, mask = XR.case_views(name)
    bad = states.copy()
    th = states[:, XR.THETA_CL, :]
    bad[:, XR.THETA_CL, :] = np.copysign(np.arccos(np.minimum(1.0, np.cos(th) * (1.0 - 1e-12))), th)
    rows, _ = XR.compare_rows(ref.states, states, bad, mask)
    assert [r.row for r in rows if not r.ok] == ["theta_cl"], [r.line() for r in rows]


@pytest.mark.parametrize("which", ["lon", "lat"])
def test_c5_changed_in_its_45th_bit_fails(which):
    """the quintic's c5 with the 45th bit of its significand flipped (2^-45 relative, at most): seen in s or d and their derivatives"""
    c = XR.case(SENS_CASE)
    lon, lat, T, tl, ref, status, cost, states = XR.coeffs_tier(SENS_CASE)
    mask = XR.compared_steps(status, c.inp.params.N + 1, c.spec.draw)
    k = {"lon": lon, "lat": lat}[which].copy()
    assert (k[:, 5] != 0).any()
    k[:, 5] = (k[:, 5].view(np.uint64) ^ np.uint64(1 << (52 - 45))).view(np.float64)
    defect, _, _ = XR.evaluate(c, (k if which == "lon" else lon).astype(LD), (k if which == "lat" else lat).astype(LD), tl)
    rows, _ = XR.compare_rows(ref.states, states, _planted(ref.states, states, defect), mask)
    assert ("s" if which == "lon" else "d") in {r.row for r in rows if not r.ok}, [r.line() for r in rows]


def test_cost_comparison_rejects_a_cost_off_in_its_twelfth_digit():
    c = XR.case(SENS_CASE)
    ref, status, cost, states, coeffs, mask = XR.case_views(SENS_CASE)
    sel = (status & 3) == 1
    e_o, e_d, bound = XR.compare_costs(ref.cost, cost, cost * (1.0 + 1e-12), sel, c.inp.params.N)
    assert e_o <= bound < e_d
    assert not XR.compare_coeffs(ref.lon, coeffs[:, :6], coeffs[:, :6] * (1.0 + 2.0 ** -40))[2]
