"""The water fixer's rule in numpy, the statement that mw_member_water_fix is held to bit for bit.

Fields are (nz, ncol, nens) fp64; a column's water is dz * sum over k of ((v + c) + r), k ascending in one accumulator that starts from
+0.0 (mw_member_column_water's order).  Every operation below is one IEEE fp64 operation of numpy, so the order is the only contract."""
import numpy as np


def column_water(v, c, r, dz):
    acc = np.zeros(v.shape[1:])
    with np.errstate(all="ignore"):
        for k in range(v.shape[0]):
            acc = acc + ((v[k] + c[k]) + r[k])
        return dz * acc


def bound(nz, w_before):
    """|W' - W_before| of a fixed column of non-negative fields: (nz + 4) * 2^-52 * W_before."""
    return (nz + 4) * 2.0 ** -52 * w_before


def water_fix(v, c, r, dz, dt, w_before, precl, rain_total, members, accum, fixed, tolerance=0.0):
    """The call on host arrays: v, c, r (nz, ncol, nens); w_before, precl, rain_total (ncol, nens).  Returns a dict of NEW arrays: v, c, r,
    precl, rain_total, excess (ncol, nens), fixed / skipped (ncol, nens) bool, counts (nens, 2) int64, sum / max (nens,) of the excess (the
    sum in numpy's order: the kernel's is another, equal where every sum is exact)."""
    nz, ncol, nens = v.shape
    assert set(fixed) <= set(members)
    v, c, r, precl, rain_total = v.copy(), c.copy(), r.copy(), precl.copy(), rain_total.copy()
    wa = column_water(v, c, r, dz)
    wb = w_before
    in_fixed = np.zeros((ncol, nens), dtype=bool)
    in_fixed[:, list(fixed)] = True
    with np.errstate(all="ignore"):
        d = wa - wb
        bad = ~np.isfinite(wa) | ~np.isfinite(wb)
        skipped = in_fixed & (bad | ((wa > wb) & (wb < 0.0)))
        fix = in_fixed & ~skipped & (wb >= 0.0) & (d > tolerance * wb)
        s = np.where(fix, wb / np.where(fix, wa, 1.0), 1.0)
        for q in (v, c, r):
            q[:, fix] = q[:, fix] * s[fix]
        w_now = np.where(fix, column_water(v, c, r, dz), wa)
        for m in members:
            precl[:, m] = (wb[:, m] - w_now[:, m]) / (1000.0 * dt)
        for m in accum:
            rain_total[:, m] = rain_total[:, m] + dt * precl[:, m]
    excess = np.where(fix, d, 0.0)
    counts = np.stack([fix.sum(axis=0), skipped.sum(axis=0)], axis=1).astype(np.int64)
    return {"v": v, "c": c, "r": r, "precl": precl, "rain_total": rain_total, "excess": excess, "fixed": fix, "skipped": skipped,
            "counts": counts, "sum": excess.sum(axis=0), "max": excess.max(axis=0), "w_after": wa, "w_now": w_now}
