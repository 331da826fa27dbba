"""numpy statement of the harvest outside the training box, on the host only: the draw, eligibility, the three classes,
the mask and the six counts of mw_member_sample_mask_domain; harvest_thresholds; the union rule of training_domain.txt.  Everything
but the thresholds is integer or bitwise: the tests compare with ==."""
import numpy as np

BEFORE = (0, 2, 3, 4)                  # the input field that teacher value v replaces, and the fields that have a level above
CLASSES = ("outside", "active", "inactive")


def u01(keys):
    """splitmix64's finaliser of uint64 keys (wrapping arithmetic), the top 53 bits as a double in [0, 1): csrc/mw_sample_key.h."""
    with np.errstate(over="ignore"):
        z = np.asarray(keys, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def f32_finite(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(np.asarray(a, dtype=np.float64).astype(np.float32))


def classify(f5, t4, members, boxes, above):
    """f5 / t4: five / four host arrays (nz, ncol, nens); members, boxes (nm, 5, 2), above (nm).  Returns flat arrays over the elements
    t = (k * ncol + col) * nens + e: row (the member's place in the list, -1: not listed), eligible (bool), cls (0 outside, 1 active,
    2 inactive; -1 where not eligible or not listed)."""
    nz, ncol, nens = f5[0].shape
    plane, nelem = ncol * nens, nz * ncol * nens
    t = np.arange(nelem, dtype=np.int64)
    up = np.where(t + plane < nelem, t + plane, t)
    f = [np.asarray(a, dtype=np.float64).ravel() for a in f5]
    g = [np.asarray(a, dtype=np.float64).ravel() for a in t4]
    row = np.full(nelem, -1, dtype=np.int64)
    for j, m in enumerate(members):
        row[t % nens == m] = j
    fin = np.ones(nelem, dtype=bool)
    for a in f:
        fin &= f32_finite(a)
    for v in BEFORE:
        fin &= f32_finite(f[v][up])
    for a in g:
        fin &= f32_finite(a)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(len(members), 5, 2)
    j = np.maximum(row, 0)
    with np.errstate(invalid="ignore"):
        out = np.zeros(nelem, dtype=bool)
        for v in range(5):
            out |= (f[v] < boxes[j, v, 0]) | (f[v] > boxes[j, v, 1])
        ab = np.asarray([bool(a) for a in above])[j]
        for v in BEFORE:
            out |= ab & ((f[v][up] < boxes[j, v, 0]) | (f[v][up] > boxes[j, v, 1]))
        act = np.zeros(nelem, dtype=bool)
        for v in range(4):
            act |= np.abs(g[v] - f[BEFORE[v]]) > 1.e-10
    eligible = fin & (row >= 0)
    cls = np.where(out, 0, np.where(act, 1, 2))
    cls[~eligible] = -1
    return row, eligible, cls


def mask_and_counts(f5, t4, members, boxes, above, key0, thr):
    """(mask (nelem,) uint8, counts (nm, 6) int64) of mw_member_sample_mask_domain; thr: (nm, 3)."""
    row, eligible, cls = classify(f5, t4, members, boxes, above)
    thr = np.asarray(thr, dtype=np.float64).reshape(len(members), 3)
    t = np.arange(row.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        draw = u01(np.uint64(int(key0) % 2 ** 64) + t)
    take = eligible & (draw < thr[np.maximum(row, 0), np.maximum(cls, 0)])
    counts = np.zeros((len(members), 6), dtype=np.int64)
    for j in range(len(members)):
        for c in range(3):
            counts[j, c] = int((eligible & (row == j) & (cls == c)).sum())
            counts[j, 3 + c] = int((take & (row == j) & (cls == c)).sum())
    return take.astype(np.uint8), counts


def sample_thresholds(want_active, want_inactive, prior_active, ncell):
    return want_active / (prior_active * ncell), want_inactive / ((1 - prior_active) * ncell)


def harvest_thresholds(samples_per_step, ratio_active, prior_active, ncell, share, eligible_outside):
    inside = (1 - share) * samples_per_step
    thr_act, thr_inact = sample_thresholds(ratio_active * inside, (1 - ratio_active) * inside, prior_active, ncell)
    thr_out = 0.0 if eligible_outside == 0 else min(1.0, share * samples_per_step / eligible_outside)
    return thr_out, min(1.0, thr_act), min(1.0, thr_inact)


def domain_union(data_in, init_rows):
    """Rows of training_domain.txt: data_in (n, n_in) this run's inputs (fp32 records), init_rows (n_in, 2) the continued model's table."""
    x = np.asarray(data_in)
    lo, hi = x.min(axis=0).astype(np.float64), x.max(axis=0).astype(np.float64)
    r = np.asarray(init_rows, dtype=np.float64)
    return np.stack([np.minimum(lo, r[:, 0]), np.maximum(hi, r[:, 1])], axis=1)
