"""The reference-table window of the single-launch kernel, without a device: the host rule (csrc/rp_table_window.h, through
lib/librp_windowtest.so) against a NumPy restatement of what a lookup of the kernels touches (tests/_window.py).

  * every s the kernel accepts for the window, [win_s_lo, win_s_hi), reads staged vertices and staged bucket entries only, and the
    lookup gives np.searchsorted(pos, s, "right");
  * the margins: the first and the last staged vertex ARE read (by windows clamped at the table's ends), and a bound one segment
    wider has a read outside the staged range -- through the bucket range; the vertex range of an unclamped window has slack, which
    the test pins as well;
  * every early return of the rule;
  * the bounds the rule takes for s(t), t in [0, T], hold (both longitudinal modes), with the margin they leave printed.
"""
import numpy as np
import pytest

import _window as W
from _window import LON_STOPPING, LON_VELOCITY_KEEPING

SIZES = (95, 96, 97, 128, 129, 255, 256, 700)
KINDS = ("uniform", "jitter", "short")


def reference(kind, n, seed=0):
    """arclengths of a reference with n vertices"""
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "uniform":
        seg = np.full(n - 1, 1.0)
    elif kind == "jitter":
        seg = rng.uniform(0.5, 2.0, n - 1)
    else:   # 10 % very short segments; as short as the bucket table allows (8192 entries at most: span / shortest segment)
        short = max(0.02, 1.25 * n / 7000.0)
        seg = np.where(rng.random(n - 1) < 0.1, short, rng.uniform(0.5, 2.0, n - 1))
    return 3.7 + np.concatenate(([0.0], np.cumsum(seg)))


def plans(pos):
    """(lon_mode, x0_lon, T, L) near the start, in the middle and near the end of the path, both modes"""
    n = len(pos)
    out = []
    for where, k in (("start", 1), ("start+", 4), ("mid", n // 2), ("end-", n - 24), ("end", n - 9)):
        s0 = float(pos[k]) + 0.31 * float(pos[k + 1] - pos[k])
        T = np.array([1.1, 2.0, 3.0])
        out.append((where, LON_VELOCITY_KEEPING, [s0, 4.0, 0.3], T, np.linspace(2.0, 6.0, 5)))
        out.append((where, LON_VELOCITY_KEEPING, [s0, 1.0, -0.2], T, np.linspace(0.0, 2.0, 3)))     # (a short window)
        out.append((where, LON_STOPPING, [s0, 5.0, -0.5], T, s0 + np.linspace(4.0, 14.0, 4)))
    return out


def probe_values(pos, lo, hi, k_from, k_to, rng, n_random=300):
    """every s in [lo, hi) of: vertex positions k_from .. k_to and their two float neighbours, lo itself, the float below hi, random ones"""
    v = pos[max(0, k_from):min(len(pos), k_to + 1)]
    s = np.concatenate((v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), [lo, np.nextafter(hi, -np.inf)], rng.uniform(lo, hi, n_random)))
    return np.unique(s[(s >= lo) & (s < hi)])


def all_windows():
    for kind in KINDS:
        for n in SIZES:
            pos = reference(kind, n)
            bk = W.bucket_table(pos)
            for where, mode, x0, T, L in plans(pos):
                yield kind, n, where, pos, bk, W.rule_window(pos, bk, mode, x0, T, L), (mode, x0, T, L)


def test_bucket_table_is_the_documented_one():
    """bucket[b] = first index with pos > pos[0] + b h, h = the shortest segment; none beyond 8192 entries"""
    for kind in KINDS:
        for n in SIZES:
            pos = reference(kind, n)
            bk = W.bucket_table(pos)
            h = np.diff(pos).min()
            want = np.floor((pos[-1] - pos[0]) / h) + 1.0
            assert want <= 8192, (kind, n, want)
            assert bk.nb == int(want) and bk.inv_h == 1.0 / h
            np.testing.assert_array_equal(bk.table, np.searchsorted(pos, pos[0] + np.arange(bk.nb) * h, "right"))
    pos = np.concatenate(([0.0], np.cumsum(np.where(np.arange(199) == 50, 1e-4, 1.0))))   # 199 m / 1e-4 m: far beyond 8192
    assert W.bucket_table(pos).nb == 0


def test_staged_reads_only_and_tight_margins():
    rng = np.random.default_rng(7)
    n_windows = first_read = last_read = 0
    wider_lo_windows = wider_lo_broken = wider_hi_windows = wider_hi_broken = 0
    bucket_rounds = 0
    slack_lo, slack_hi = 10 ** 6, 10 ** 6   # unclamped windows: vertices between the staged range's ends and the reads
    n_unclamped = wider_by_vertex = 0
    seen = set()
    for kind, n, where, pos, bk, w, _ in all_windows():
        if w.n == 0:
            continue
        n_windows += 1
        seen.add((kind, n, where))
        assert w.n == 1 << w.shift and w.n in (16, 32, 64, 128) and 0 <= w.k0 and w.k0 + w.n <= n and 2 * w.n <= n
        assert 0 <= w.b0 and w.nb >= 1 and w.b0 + w.nb <= bk.nb
        bucket_rounds = max(bucket_rounds, (w.nb + W.RP_BLOCK - 1) // W.RP_BLOCK)
        s = probe_values(pos, w.s_lo, w.s_hi, w.k0 - 3, w.k0 + w.n + 3, rng)
        assert len(s) > 100
        r = W.lookup_reads(pos, bk, s)
        tag = f"{kind} n={n} {where} window [{w.k0}, {w.k0 + w.n}) buckets [{w.b0}, {w.b0 + w.nb})"
        np.testing.assert_array_equal(r.ub, np.searchsorted(pos, s, "right"), err_msg=tag)
        assert r.vmin.min() >= w.k0 and r.vmax.max() < w.k0 + w.n, (tag, int(r.vmin.min()), int(r.vmax.max()))
        assert r.bucket.min() >= w.b0 and r.bucket.max() < w.b0 + w.nb, (tag, int(r.bucket.min()), int(r.bucket.max()))
        first_read += int((r.vmin == w.k0).sum())
        last_read += int((r.vmax == w.k0 + w.n - 1).sum())
        if w.k0 > 0 and w.k0 + w.n < n:
            n_unclamped += 1
            slack_lo, slack_hi = min(slack_lo, int(r.vmin.min()) - w.k0), min(slack_hi, w.k0 + w.n - 1 - int(r.vmax.max()))
        # one segment wider at either end (only where the bound is a vertex of the window's inside, not the end of the table)
        if w.k0 > 0:
            wider_lo_windows += 1
            s2 = probe_values(pos, pos[w.k0 + 1], w.s_lo, w.k0 - 3, w.k0 + 4, rng)
            r2 = W.lookup_reads(pos, bk, s2)
            wider_lo_broken += int(r2.vmin.min() < w.k0 or r2.bucket.min() < w.b0)
            wider_by_vertex += int(r2.vmin.min() < w.k0)
        if w.k0 + w.n < n:
            wider_hi_windows += 1
            s2 = probe_values(pos, w.s_hi, pos[w.k0 + w.n - 3], w.k0 + w.n - 6, w.k0 + w.n + 3, rng)
            r2 = W.lookup_reads(pos, bk, s2)
            wider_hi_broken += int(r2.vmax.max() >= w.k0 + w.n or r2.bucket.max() >= w.b0 + w.nb)
            wider_by_vertex += int(r2.vmax.max() >= w.k0 + w.n)
    print(f"table window, host: {n_windows} windows; reads of the first staged vertex {first_read}, of the last {last_read}; "
          f"win_s_lo one segment earlier: a read outside in {wider_lo_broken} of {wider_lo_windows} windows; "
          f"win_s_hi one segment later: {wider_hi_broken} of {wider_hi_windows} ({wider_by_vertex} of all these through a vertex, the others through "
          f"the bucket range); bucket copy loop up to {bucket_rounds} rounds; {n_unclamped} unclamped windows: the lowest read is {slack_lo} above "
          f"the first staged vertex, the highest {slack_hi} below the last")
    # the cases asked for are among the windows: every size from 96 on, every kind, start / middle / end
    for kind in KINDS:
        for n in SIZES[1:]:
            assert {wh for (k, m, wh) in seen if k == kind and m == n} >= {"start", "mid", "end"}, (kind, n)
    assert bucket_rounds > 1
    assert first_read > 0 and last_read > 0
    assert wider_lo_broken > 0 and wider_hi_broken > 0
    # What is tight is the BUCKET range (computed from the bounds, one entry of slack each way) and the two clamped ends of the vertex
    # range (a window at the start of the table reads vertex 0, one at its end vertex n - 1).  The vertex range of a window clamped at
    # neither end has slack: a lookup in segment seg reads vertices seg - 1 .. seg + 2 (one step back, two forward), not the
    # seg - 2 .. seg + 3 the rule allows for.  A bound one segment wider, with the bucket range computed from it, therefore still
    # reads staged entries only -- which is why the device tests cannot tell such a rule from the shipped one.
    assert n_unclamped > 50 and slack_lo == 1 and slack_hi >= 2 and wider_by_vertex == 0


def test_first_valid_segment():
    """Which staged segment can a VALID step (s between the rule's lo and hi) lie in?  The rule puts w0 = seg_lo - 3 and the window
    accepts s from pos[w0 + 2] on: segment w0 + 2 is reached only when w0 was clamped (at the start of the table, or moved down by the
    clamp at its end); otherwise the first one is w0 + 3."""
    unclamped = clamped = 0
    for kind, n, where, pos, bk, w, (mode, x0, T, L) in all_windows():
        if w.n == 0:
            continue
        lo, hi = rule_bounds(mode, x0, T, L)
        seg_lo = int(np.searchsorted(pos, lo, "right")) - 1
        seg_hi = int(np.searchsorted(pos, hi, "right")) - 1
        if w.k0 + w.n < n and w.k0 > 0:
            assert w.k0 == seg_lo - 3        # first valid segment: w0 + 3
            assert seg_hi <= w.k0 + w.n - 5  # last admissible one
            unclamped += 1
        else:
            assert w.k0 <= max(0, seg_lo - 3)
            clamped += 1
    assert unclamped > 0 and clamped > 0


def test_early_returns():
    pos = reference("uniform", 256)
    bk = W.bucket_table(pos)
    x0 = [float(pos[100]) + 0.5, 4.0, 0.2]
    T, L = np.array([1.0, 3.0]), np.array([2.0, 6.0])
    ok = W.rule_window(pos, bk, LON_VELOCITY_KEEPING, x0, T, L)
    assert ok.n == 32 and ok.k0 == 100 - 3                     # 0 .. 18 m ahead: segments 100 .. 118, + 8 = 27 vertices
    assert ok.s_lo == pos[ok.k0 + 2] and ok.s_hi == pos[ok.k0 + ok.n - 4]
    whole = W.Window(0, 0, 0, 0, 0, 0.0, 0.0)
    # n < 96
    p95 = reference("uniform", 95)
    assert W.rule_window(p95, W.bucket_table(p95), LON_VELOCITY_KEEPING, [float(p95[40]), 1.0, 0.0], T, np.array([1.0])) == whole
    p96 = reference("uniform", 96)
    assert W.rule_window(p96, W.bucket_table(p96), LON_VELOCITY_KEEPING, [float(p96[40]), 1.0, 0.0], T, np.array([1.0])).n == 16
    assert W.lib().rptw_test_constant(0) == 96 and W.lib().rptw_test_constant(1) == 128 and W.lib().rptw_test_constant(2) == 8192
    # no bucket table
    assert W.rule_window(pos, W.Buckets(bk.table, 0, bk.inv_h), LON_VELOCITY_KEEPING, x0, T, L) == whole
    fine = np.concatenate(([0.0], np.cumsum(np.where(np.arange(255) == 7, 1e-4, 1.0))))
    bf = W.bucket_table(fine)
    assert bf.nb == 0 and W.rule_window(fine, bf, LON_VELOCITY_KEEPING, [100.5, 4.0, 0.2], T, L) == whole
    # empty T or L
    assert W.rule_window(pos, bk, LON_VELOCITY_KEEPING, x0, np.array([]), L) == whole
    assert W.rule_window(pos, bk, LON_VELOCITY_KEEPING, x0, T, np.array([])) == whole
    # NaN or infinite samples, in either mode
    for mode in (LON_VELOCITY_KEEPING, LON_STOPPING):
        base_L = L if mode == LON_VELOCITY_KEEPING else x0[0] + np.array([5.0, 10.0])
        assert W.rule_window(pos, bk, mode, x0, T, base_L).n > 0
        for bad in (np.inf, -np.inf):
            assert W.rule_window(pos, bk, mode, x0, T, np.append(base_L, bad)) == whole, (mode, bad)
            assert W.rule_window(pos, bk, mode, x0, np.append(T, bad), base_L) == whole or bad == -np.inf, (mode, bad)
            assert W.rule_window(pos, bk, mode, [x0[0], bad, 0.0], T, base_L) == whole, (mode, bad)
        # NaN: a NaN start position is refused in both modes, NaN anywhere in the stopping bound's overshoot term as well.  The
        # rule's minima and maxima (std::min / std::max) pass a NaN over wherever it is the second argument, so that a NaN sample
        # elsewhere leaves the window of the other samples (or a narrower one): never a range outside the table, and the kernel's own
        # check -- NaN lies in no interval -- sends the workgroups of such pairs to the whole block (_window.classify counts them so).
        nan = np.nan
        assert W.rule_window(pos, bk, mode, [nan, 4.0, 0.2], T, base_L) == whole
        if mode == LON_STOPPING:
            for bad in (([x0[0], nan, 0.2], T, base_L), ([x0[0], 4.0, nan], T, base_L), (x0, np.append(nan, T), base_L)):
                assert W.rule_window(pos, bk, mode, *bad) == whole
        for bad in ((x0, T, np.append(nan, base_L)), (x0, T, np.append(base_L, nan)), (x0, np.append(nan, T), base_L), (x0, np.append(T, nan), base_L),
                    ([x0[0], nan, 0.2], T, base_L), ([x0[0], 4.0, nan], T, base_L)):
            w = W.rule_window(pos, bk, mode, *bad)
            assert w == whole or (w.n in (16, 32, 64, 128) and 0 <= w.k0 and w.k0 + w.n <= len(pos) and 0 <= w.b0 and w.b0 + w.nb <= bk.nb
                                  and pos[w.k0] <= w.s_lo <= w.s_hi <= pos[w.k0 + w.n - 1]), (mode, bad, w)
    # wider than n / 2 (n = 96: 48 vertices; 30 segments + 8 need 64) and wider than 128 vertices (n = 700: 125 segments + 8 need 256)
    assert W.rule_window(p96, W.bucket_table(p96), LON_VELOCITY_KEEPING, [float(p96[10]), 10.0, 0.0], T, np.array([10.0])) == whole
    p700 = reference("uniform", 700)
    b700 = W.bucket_table(p700)
    assert W.rule_window(p700, b700, LON_VELOCITY_KEEPING, [float(p700[100]) + 0.5, 40.0, 0.0], T, np.array([39.9])).n == 128    # 120 segments
    assert W.rule_window(p700, b700, LON_VELOCITY_KEEPING, [float(p700[100]) + 0.5, 41.0, 0.0], T, np.array([41.0])) == whole    # 123 + 8 > 128
    # the clamp w0 = n - wn: the window ends with the table, and with it win_s_hi is the last vertex
    w = W.rule_window(pos, bk, LON_VELOCITY_KEEPING, [float(pos[240]) + 0.5, 4.0, 0.2], T, L)
    assert w.n == 32 and w.k0 == 256 - 32 and w.s_hi == pos[-1] and w.s_lo == pos[w.k0 + 2] and w.b0 + w.nb == bk.nb
    # ... and w0 == 0: win_s_lo is the first vertex
    w = W.rule_window(pos, bk, LON_VELOCITY_KEEPING, [float(pos[1]) + 0.5, 4.0, 0.2], T, L)
    assert w.k0 == 0 and w.s_lo == pos[0] and w.b0 == 0 and w.s_hi == pos[w.n - 4]


def rule_bounds(mode, x0, T, L):
    """[lo, hi] of csrc/rp_table_window.h, restated (test_first_valid_segment holds it against the library's window)"""
    s0, v0, a0 = x0[0], x0[1], abs(x0[2])
    Tmax, Lmin, Lmax = np.max(T), np.min(L), np.max(L)
    if mode == LON_STOPPING:
        over = 0.2 * abs(v0) * Tmax + 0.0173 * a0 * Tmax * Tmax
        return min(s0, Lmin) - over, max(s0, Lmax) + over
    dv = (4.0 / 27.0) * Tmax * a0
    return s0 + min(0.0, (min(v0, Lmin) - dv) * Tmax), s0 + max(0.0, (max(v0, Lmax) + dv) * Tmax)


def test_bounds_hold_for_valid_steps():
    """s(t), t in [0, T], stays inside [lo, hi] for single (T, sample) pairs -- the rule's bounds for a grid are the union over its
    pairs with T replaced by the largest.  The stopping bound's 0.2 and 0.0173 stand for the maxima of two quintic Hermite basis
    functions, tau (1 - tau)^3 (1 + 3 tau) (0.1976 at tau = 1/3 ...) and tau^2 (1 - tau)^3 / 2 (0.01728 at tau = 2/5): 1.2 % and
    0.1 % above them.  4001 samples of t resolve the maximum of a quintic to ~1e-7 of its value."""
    tau = np.linspace(0.0, 1.0, 4001)
    B, Cc = tau * (1 - tau) ** 3 * (1 + 3 * tau), 0.5 * tau ** 2 * (1 - tau) ** 3
    print(f"quintic Hermite basis maxima: {B.max():.6f} (rule: 0.2), {Cc.max():.6f} (rule: 0.0173)")
    assert 0.197 < B.max() < 0.2 and 0.01727 < Cc.max() < 0.0173
    rng = np.random.default_rng(11)
    worst = {LON_VELOCITY_KEEPING: np.inf, LON_STOPPING: np.inf}
    for mode in (LON_VELOCITY_KEEPING, LON_STOPPING):
        for k in range(4000):
            s0, T = rng.uniform(-50.0, 500.0), rng.uniform(0.3, 8.0)
            v0, a0 = rng.uniform(-2.0, 30.0), rng.uniform(-6.0, 6.0)
            if k % 4 == 0:    # the terms one at a time: only v0 / only a0 pushes s beyond the end points
                v0, a0 = (v0, 0.0) if k % 8 == 0 else (0.0, a0)
            sample = rng.uniform(0.0, 30.0) if mode == LON_VELOCITY_KEEPING else s0 + (0.0 if k % 4 == 0 else rng.uniform(-5.0, 80.0))
            c = W.lon_coeffs(mode, [s0, v0, a0], T, sample)
            s = W.poly_pos(c, tau * T)
            lo, hi = rule_bounds(mode, [s0, v0, a0], np.array([T]), np.array([sample]))
            scale = abs(v0) * T + abs(a0) * T * T + 1e-9
            m = min(hi - s.max(), s.min() - lo)
            assert m >= -1e-9 * (abs(s0) + scale), (mode, s0, v0, a0, T, sample, m)
            worst[mode] = min(worst[mode], m / scale)
    print(f"smallest margin of the rule's bounds over s(t), relative to |v0| T + |a0| T^2: velocity keeping {worst[LON_VELOCITY_KEEPING]:.3e}, "
          f"stopping {worst[LON_STOPPING]:.3e}")
