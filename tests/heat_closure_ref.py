"""The latent-heat closure's rule in numpy, the statement that mw_member_heat_closure is held to bit for bit, and the
order of its sums.

Fields are (nz, ncol, nens) fp64.  Per cell of a diagnosed member, every line one IEEE fp64 operation of numpy:
    C   = lv / cp_d
    T_c = temp_before + C * ((rho_v_before - rho_v_after) / rho_d)
    r   = temp_after - T_c
r not finite: skipped (counted, temp untouched, out of every sum); member closed and |r| > tolerance: temp = T_c; else nothing.
A column's sums (r, |r|, r * r, max |r|, rho_d * r) run over k ascending from +0.0; H = ((cp_d * dz) / dt) * sum_k rho_d * r.
`closure` returns the per-member sums in numpy's order; `kernel_order_stats` restates the kernels' order: a block of 256 consecutive plane
elements t = col * nens + e folds each member's lanes in ascending order from +0.0, thread l of 256 folds the blocks l, l + 256, ... in
ascending order from +0.0, and the 256 results are folded in ascending l."""
import numpy as np

LV, CP_D = 2.5e6, 1003.0


def ulp(x):
    """The spacing of fp64 at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


KESSLER_CASES = [(40, 64, 500.0, 1.0), (40, 64, 100.0, 30.0), (8, 64, 50.0, 60.0)]        # (nz, ncol, dz, dt)


def moist_state(nz, ncol, dz, seed):
    """{rho_d, temp, rho_v, rho_c, rho_r}: (nz, ncol) random moist columns on a standard profile (300 K at the ground, 6.5 K / km, never
    below 210 K; pressure 1e5 exp(-z / 8000)): vapour 0 .. 1.3 of Tetens' saturation mixing ratio, and in half the cells cloud up to 3e-3
    and rain up to 8e-3 kg / kg."""
    rng = np.random.default_rng(seed)
    z = ((np.arange(nz) + 0.5) * dz)[:, None]
    temp = np.maximum(300.0 - 6.5e-3 * z, 210.0) + rng.uniform(-2.0, 2.0, (nz, ncol))
    p = 1.0e5 * np.exp(-z / 8000.0)
    rho_d = p / (287.0 * temp)
    qvs = 380.0 / p * np.exp(17.27 * (temp - 273.0) / (temp - 36.0))
    wet = rng.uniform(0.0, 1.0, (nz, ncol)) < 0.5
    return {"rho_d": rho_d, "temp": temp, "rho_v": rng.uniform(0.0, 1.3, (nz, ncol)) * qvs * rho_d,
            "rho_c": np.where(wet, rng.uniform(0.0, 3.0e-3, (nz, ncol)), 0.0) * rho_d,
            "rho_r": np.where(wet, rng.uniform(0.0, 8.0e-3, (nz, ncol)), 0.0) * rho_d}


def kessler_bound(rainsplit, temp):
    """|r| of a cell of a Kessler step: (rainsplit + 4) ulp(temp) -- one rounding of theta per rain sub-cycle, temp / exner, theta * exner
    and the closure's own two roundings (the vapour side is 1e-2 of that)."""
    return (rainsplit + 4) * ulp(temp)


def residual(temp_after, rho_d, rho_v_after, temp_before, rho_v_before, lv=LV, cp_d=CP_D):
    """(T_c, r) of every cell."""
    C = lv / cp_d
    with np.errstate(all="ignore"):
        tc = temp_before + C * ((rho_v_before - rho_v_after) / rho_d)
        return tc, temp_after - tc


def closure(temp_after, rho_d, rho_v_after, temp_before, rho_v_before, dz, dt, members, closed, tolerance=0.0, lv=LV, cp_d=CP_D):
    """The call on host arrays.  Returns a dict of NEW arrays: temp (nz, ncol, nens); r, T_c (every cell, whatever its member); closed_cells,
    skipped_cells (nz, ncol, nens) bool; counts (nens, 2) int64; lanes (ncol, nens, 6) = every column's sum r, sum |r|, sum r^2, max |r|, H,
    |H| (zeros for a member not diagnosed); heating (ncol, nens) = H; stats (nens, 6) in numpy's order; max_r, max_h (nens,)."""
    nz, ncol, nens = temp_after.shape
    assert set(closed) <= set(members)
    listed = np.zeros(nens, dtype=bool)
    listed[list(members)] = True
    closes = np.zeros(nens, dtype=bool)
    closes[list(closed)] = True
    tc, r = residual(temp_after, rho_d, rho_v_after, temp_before, rho_v_before, lv, cp_d)
    finite = np.isfinite(r)
    skipped = ~finite & listed
    with np.errstate(all="ignore"):
        hit = finite & closes & (np.abs(r) > tolerance)
        temp = np.where(hit, tc, temp_after)
        lanes = np.zeros((ncol, nens, 6))
        h = np.zeros((ncol, nens))
        for k in range(nz):
            ok = finite[k] & listed
            rk = np.where(ok, r[k], 0.0)
            lanes[..., 0] = np.where(ok, lanes[..., 0] + rk, lanes[..., 0])
            lanes[..., 1] = np.where(ok, lanes[..., 1] + np.abs(rk), lanes[..., 1])
            lanes[..., 2] = np.where(ok, lanes[..., 2] + rk * rk, lanes[..., 2])
            lanes[..., 3] = np.where(ok & (np.abs(rk) > lanes[..., 3]), np.abs(rk), lanes[..., 3])
            h = np.where(ok, h + np.where(ok, rho_d[k], 0.0) * rk, h)
        scale = cp_d * dz / dt
        heating = np.where(listed, scale * h, 0.0)
        lanes[..., 4] = heating
        lanes[..., 5] = np.abs(heating)
        stats = np.stack([lanes[..., 0].sum(axis=0), lanes[..., 1].sum(axis=0), lanes[..., 2].sum(axis=0), lanes[..., 3].max(axis=0),
                          lanes[..., 4].sum(axis=0), lanes[..., 5].max(axis=0)], axis=1)
    counts = np.stack([hit.sum(axis=(0, 1)), skipped.sum(axis=(0, 1))], axis=1).astype(np.int64)
    return {"temp": temp, "r": r, "T_c": tc, "closed_cells": hit, "skipped_cells": skipped, "counts": counts, "lanes": lanes,
            "heating": heating, "stats": stats, "max_r": stats[:, 3].copy(), "max_h": stats[:, 5].copy()}


def kernel_order_stats(lanes):
    """(nens, 6) from closure()'s `lanes` (ncol, nens, 6) in the kernels' order of folding."""
    ncol, nens, _ = lanes.shape
    flat = lanes.reshape(ncol * nens, 6)
    plane = ncol * nens
    nblocks = (plane + 255) // 256
    is_max = (3, 5)
    rows = np.zeros((nblocks, nens, 6))
    for b in range(nblocks):
        for m in range(nens):
            first = (m - (b * 256) % nens + nens) % nens
            acc = np.zeros(6)
            for j in range(first, 256, nens):
                t = b * 256 + j
                if t >= plane:
                    break
                for c in range(6):
                    acc[c] = max(acc[c], flat[t, c]) if c in is_max else acc[c] + flat[t, c]
            rows[b, m] = acc
    out = np.zeros((nens, 6))
    for m in range(nens):
        part = np.zeros((256, 6))
        for lane in range(min(256, nblocks)):
            for b in range(lane, nblocks, 256):
                for c in range(6):
                    part[lane, c] = max(part[lane, c], rows[b, m, c]) if c in is_max else part[lane, c] + rows[b, m, c]
        acc = part[0].copy()
        for lane in range(1, 256):
            for c in range(6):
                acc[c] = max(acc[c], part[lane, c]) if c in is_max else acc[c] + part[lane, c]
        out[m] = acc
    return out
