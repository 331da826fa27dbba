"""The training-domain guard stated in numpy: the box of a model or a committee from the rows of the input scaling
tables, and the classification of a member-fastest state against per-member boxes -- counts (nm, 16), flags and the newly flagged
counts per slot, as mw_member_domain leaves them.  Everything is integer or bitwise: the tests compare with ==."""
import numpy as np

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
ABOVE_ROW = {0: 5, 2: 6, 3: 7, 4: 8}       # a stencil model's row of the level above, per field that has one


def box_of(tables, margin=0.0, fields=IN5):
    """tables: the models' scl_in arrays, all (5, 2) or all (9, 2).  -> (5, 2) fp64; ValueError naming the field when an intersection is
    empty.  The margin arithmetic is the written formula, in fp64: [lo - m * w, hi + m * w] with w = hi - lo."""
    tables = [np.asarray(t, dtype=np.float64) for t in tables]
    out = np.empty((5, 2), dtype=np.float64)
    m = np.float64(margin)
    for f, name in enumerate(IN5):
        if name not in fields:
            out[f] = (-np.inf, np.inf)
            continue
        lo = max(t[f, 0] for t in tables)
        hi = min(t[f, 1] for t in tables)
        if tables[0].shape[0] == 9 and f in ABOVE_ROW:
            lo = max([lo] + [t[ABOVE_ROW[f], 0] for t in tables])
            hi = min([hi] + [t[ABOVE_ROW[f], 1] for t in tables])
        if hi < lo:
            raise ValueError("empty box for %s" % name)
        w = np.float64(hi) - np.float64(lo)
        out[f] = (np.float64(lo) - m * w, np.float64(hi) + m * w)
    return out


def classify(in5, members, boxes, flags=None, slots=None, flag_counts=None):
    """in5: five host arrays (nz, ncol, nens); boxes (nm, 5, 2).  -> counts (nm, 16) int64; with flags ((ncol, nens) uint8), slots and
    flag_counts ((slots, 2) int64) also (flags after, flag_counts after) -- copies; the inputs stay as they are."""
    nz, ncol, nens = in5[0].shape
    boxes = np.asarray(boxes, dtype=np.float64).reshape(len(members), 5, 2)
    counts = np.zeros((len(members), 16), dtype=np.int64)
    flags = None if flags is None else np.array(flags, dtype=np.uint8).reshape(ncol, nens).copy()
    flag_counts = None if flag_counts is None else np.array(flag_counts, dtype=np.int64).copy()
    for j, e in enumerate(members):
        outside = np.zeros(ncol, dtype=bool)
        for f in range(5):
            x = in5[f][:, :, e]
            with np.errstate(invalid="ignore"):
                below, above, nan = x < boxes[j, f, 0], x > boxes[j, f, 1], x != x
            counts[j, 3 * f], counts[j, 3 * f + 1], counts[j, 3 * f + 2] = below.sum(), above.sum(), nan.sum()
            outside |= (below | above | nan).any(axis=0)
        counts[j, 15] = outside.sum()
        if flags is not None and slots is not None and slots[j] >= 0:
            new = outside & (flags[:, e] == 0)
            flags[outside, e] = 1
            flag_counts[slots[j], 0] += new.sum()
            flag_counts[slots[j], 1] += new.sum()
    return (counts, flags, flag_counts) if flags is not None else counts
