"""The numpy reference of mw_surrogate_eval_domain: which cells lie outside a model's box, which are active, and the
statistics of d = prediction - truth per (side, class, field) with the bound of a fixed-order fp64 sum.  Pure numpy: no GPU, no library.

A cell is outside for a model iff some tested value x fails lo <= x && x <= hi against the model's row of x's field: NaN is outside, a
bound is inside, -0.0 is inside lo = 0.0, +-inf is inside an infinite bound.  Tested: the cell's five inputs; for a model of width 9 also
temp, water_vapor, cloud_liquid, precip_liquid of level min(nz - 1, k + 1) of the same column, against the same rows."""
import math

import numpy as np

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
BEFORE = (0, 2, 3, 4)                      # the input field that output v replaces
ABOVE = (0, 2, 3, 4)                       # the fields whose level above a model of width 9 reads


def outside_mask(n_in, ins, box):
    """ins: five arrays (nz, ncol); box (5, 2).  Returns bool (nz, ncol)."""
    box = np.asarray(box, dtype=np.float64)
    bad = np.zeros(np.shape(ins[0]), bool)
    with np.errstate(invalid="ignore"):
        for f in range(5):
            x = np.asarray(ins[f])
            bad |= ~((box[f, 0] <= x) & (x <= box[f, 1]))
        if n_in == 9:
            for f in ABOVE:
                x = np.asarray(ins[f])
                up = np.concatenate([x[1:], x[-1:]], axis=0)               # the top level is its own level above
                bad |= ~((box[f, 0] <= up) & (up <= box[f, 1]))
    return bad


def active_mask(ins, truth):
    act = np.zeros(np.shape(ins[0]), bool)
    with np.errstate(invalid="ignore"):
        for v in range(4):
            act |= np.abs(np.asarray(truth[v]) - np.asarray(ins[BEFORE[v]])) > 1e-10
    return act


def _sum(terms):
    """The exactly rounded sum (math.fsum); with a non-finite term what any order of fp64 additions gives: NaN, or the infinity."""
    if terms.size and not np.all(np.isfinite(terms)):
        with np.errstate(invalid="ignore"):
            return float(np.sum(terms))
    return math.fsum(terms)


def host_stats(pred, truth, outside, act):
    """(stats (2, 2, 4, 4), bound (2, 2, 4, 3), counts (2, 2)) = [side][class][field] of one prediction (four arrays): exactly rounded sums
    of d, |d|, d^2 and the maximum of |d| (NaN if some |d| is); bound = n * 2^-52 * sum |terms| with n the cells of the (side, class)."""
    stats, bound = np.zeros((2, 2, 4, 4)), np.zeros((2, 2, 4, 3))
    counts = np.zeros((2, 2), dtype=np.int64)
    outside, act = np.ravel(outside), np.ravel(act)
    for sd, side in enumerate((~outside, outside)):
        for c, cls in enumerate((~act, act)):
            sel = side & cls
            counts[sd, c] = np.count_nonzero(sel)
            for v in range(4):
                with np.errstate(invalid="ignore", over="ignore"):
                    d = (np.ravel(pred[v]) - np.ravel(truth[v]))[sel]
                    terms = (d, np.abs(d), d * d)
                for s in range(3):
                    stats[sd, c, v, s] = _sum(terms[s])
                stats[sd, c, v, 3] = np.max(np.abs(d)) if d.size else 0.0      # (np.max: NaN if any)
                bound[sd, c, v] = counts[sd, c] * 2.0 ** -52 * stats[sd, c, v, [1, 1, 2]]
    return stats, bound, counts


def model_rows(n_in, ins, truth, pred, box):
    """One model's reference: (stats (2, 2, 2, 4, 4) = [prediction | persistence][side][class][field][statistic], bound (2, 2, 2, 4, 3),
    counts (2, 2))."""
    out, act = outside_mask(n_in, ins, box), active_mask(ins, truth)
    s0, b0, cnt = host_stats(pred, truth, out, act)
    s1, b1, _ = host_stats([ins[i] for i in BEFORE], truth, out, act)
    return np.stack([s0, s1]), np.stack([b0, b1]), cnt


def np_strict_forward(X, net, form="state"):
    """The strict kernels' cell on a feature matrix X (n_in, cells) of either width: fp32 in index order, one rounding per operation, the
    quotient form of the scaling; form "tendency": y = X[base] + (o * rng + min) in fp64, base = rows 0, 2, 3, 4.  The clip is the
    device's fmax(0, y), which returns 0 for a NaN y (np.fmax)."""
    W1, b1, W2, b2, si, so = net[:6]
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((X - si[:, 0:1]) / (si[:, 1:2] - si[:, 0:1])).astype(np.float32)
        W1, b1, W2, b2 = [np.asarray(a, np.float32) for a in (W1, b1, W2, b2)]
        h = []
        for o in range(10):
            acc = np.zeros(x.shape[1], np.float32)
            for i in range(x.shape[0]):
                acc = acc + x[i] * W1[i, o]
            acc = acc + b1[o]
            h.append(np.where(acc > 0, acc, np.float32(0.1) * acc))
        outs = []
        for o in range(4):
            acc = np.zeros(x.shape[1], np.float32)
            for i in range(10):
                acc = acc + h[i] * W2[i, o]
            acc = acc + b2[o]
            assert acc.dtype == np.float32
            y = acc.astype(np.float64) * (so[o, 1] - so[o, 0]) + so[o, 0]
            if form == "tendency":
                y = X[BEFORE[o]] + y
            outs.append(y if o == 0 else np.fmax(0.0, y))
    return outs
