"""The committee's combination rule in numpy (no GPU, no library): what mw_surrogate_committee_apply computes from its members' outputs.

For one output field, ys[j] is member j's output (the bits the forward kernels store), all of one shape:
    mean  = (((ys[0] + ys[1]) + ys[2]) + ...) / float(n)       fp64, in the order given, one rounding per operation
    range = hi - lo                                            hi / lo: the largest / smallest member, NaN where any member is
numpy adds and divides float64 arrays element by element in IEEE arithmetic and never contracts, so the loop below IS the rule."""
import numpy as np


def nan_max(a, b):
    """The larger of a and b, NaN where either is (the kernels' eval_max: b wins when it is larger or NaN, a NaN a is never beaten)."""
    return np.where((b > a) | np.isnan(b), b, a)


def nan_min(a, b):
    return np.where((b < a) | np.isnan(b), b, a)


def combine(ys):
    """(mean, range) of the members' outputs ys (a sequence of n float64 arrays of one shape), in the order of the sequence."""
    ys = [np.asarray(y, dtype=np.float64) for y in ys]
    if not ys:
        raise ValueError("a committee has at least one member")
    s, hi, lo = ys[0].copy(), ys[0].copy(), ys[0].copy()
    for y in ys[1:]:
        s = s + y
        hi = nan_max(hi, y)
        lo = nan_min(lo, y)
    with np.errstate(invalid="ignore"):
        return s / np.float64(len(ys)), hi - lo


def same_bits(a, b):
    """Equal shapes and equal bits, except that any NaN equals any NaN (the payload and sign of a NaN that arithmetic produced differ
    between processors; where it is, does not)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))
