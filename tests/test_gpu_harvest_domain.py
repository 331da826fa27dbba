"""Harvest outside the training box and the domain table that follows --init, on the GPU: mw_member_sample_mask_domain
against the numpy statement of harvest_domain_ref and against mw_member_sample_mask, the harvester's two-call sequence, the rollout and
the driver with `harvest.outside`, and training_domain.txt through three trainings and into a rollout's box.

Mask bytes and count words are compared with ==.  The kernel is one element per thread in blocks of 256: the shapes sit on the block tail
(1, 256, 257, 258, 255 and 1040 elements), on the plane boundary of `up` and on the member interleave."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import harvest_domain_ref as ref

pytestmark = pytest.mark.gpu

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
BEFORE = ref.BEFORE
SHAPES = [(1, 1, 1), (2, 128, 1), (1, 257, 1), (3, 43, 2), (5, 17, 3), (4, 65, 4)]
BOX = np.array([[250.0, 300.0], [-math.inf, math.inf], [0.001, 0.01], [0.0, 0.002], [0.0, 0.005]])      # density_dry: an infinite bound
INF_BOX = np.tile(np.array([[-math.inf, math.inf]]), (5, 1))


def member_lists(nens):
    lists = [list(range(nens))] + ([[nens - 1]] if nens > 1 else [])
    return lists + ([[3, 1]] if nens > 3 else [])


def cases():
    return [pytest.param(s, m, id="%s-%s" % ("x".join(map(str, s)), "".join(map(str, m)))) for s in SHAPES for m in member_lists(s[2])]


def boxes_for(nm):
    """One box per listed member: BOX, narrower by 4 % of its width per place in the list (the infinite bounds stay)."""
    out = np.tile(BOX, (nm, 1, 1))
    w = np.where(np.isfinite(BOX[:, 1] - BOX[:, 0]), BOX[:, 1] - BOX[:, 0], 0.0)
    for j in range(nm):
        out[j, :, 1] -= 0.04 * j * w
    out[:, 4, 0] = 0.0
    return out


def base_state(nz, ncol, nens, seed):
    """Host fields strictly inside BOX's narrowest version (density_dry in [0.2, 1.2]) and teacher values: about 40 % of the elements
    active, about 15 % pushed outside the box through one field."""
    rng = np.random.default_rng(seed)
    shape = (nz, ncol, nens)
    lo = np.array([250.0, 0.2, 0.001, 0.0, 0.0])
    hi = np.array([260.0, 1.2, 0.005, 0.001, 0.002])
    f5 = [lo[v] + (hi[v] - lo[v]) * rng.uniform(0.05, 0.95, shape) for v in range(5)]
    out = rng.random(shape) < 0.15
    which = rng.integers(0, 4, size=shape)
    f5[0][out & (which == 0)] = 301.0                                          # above
    f5[2][out & (which == 1)] = 0.0005                                         # below
    f5[3][out & (which == 2)] = -1.0e-9                                        # below a zero bound
    f5[4][out & (which == 3)] = 0.0051                                         # above
    t4 = [f5[v].copy() for v in BEFORE]
    moved = rng.random(shape) < 0.4
    pick = rng.integers(0, 4, size=shape)
    for v in range(4):
        t4[v][moved & (pick == v)] += 1.0e-3 * (1.0 if v == 0 else 1.0e-3)
    return f5, t4


def plant(f5, t4, members, boxes):
    """Bound, one-beyond-the-bound and non-finite values at level 0, at the top level and in the level above a tested cell, for every listed
    member, at columns of their own where the shape has them.  Returns what it planted: (what, level, column, member)."""
    nz, ncol, nens = f5[0].shape
    log, col = [], [0]

    def at(what, arr, k, e, value):
        if not 0 <= k < nz:
            return
        c = col[0] % ncol
        col[0] += 1
        arr[k, c, e] = value
        log.append((what, k, c, e))
    for j, e in enumerate(members):
        b = boxes[j]
        for k in (0, nz - 1, 1):                                               # (level 1: the level above level 0's cell)
            at("at lo", f5[0], k, e, b[0, 0])
            at("at hi", f5[2], k, e, b[2, 1])
            at("below lo", f5[0], k, e, np.nextafter(b[0, 0], -np.inf))
            at("above hi", f5[3], k, e, np.nextafter(b[3, 1], np.inf))
            at("-0.0 at lo = 0", f5[4], k, e, -0.0)
            at("infinite bound", f5[1], k, e, 1.0e30)
            at("nan input", f5[2], k, e, np.nan)
            at("inf input", f5[1], k, e, np.inf)
            at("1e300 input", f5[4], k, e, 1.0e300)
            at("nan teacher", t4[0], k, e, np.nan)
            at("inf teacher", t4[3], k, e, -np.inf)
            at("1e300 teacher", t4[1], k, e, -1.0e300)
    return log


def to_device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def device_call(df5, dt4, members, boxes, above, key0, thr, with_mask=True, counts_fill=-12345):
    """mw_member_sample_mask_domain through modules.member_sample_mask_domain with a sentinel-filled mask and preset counts: (mask, counts)."""
    import torch
    from miniweatherml_amd import modules
    nz = df5[0].shape[0]
    mask = torch.full((df5[0].numel(),), 7, dtype=torch.uint8, device="cuda")
    counts = torch.full((len(members), 6), counts_fill, dtype=torch.int64, device="cuda")
    got = modules.member_sample_mask_domain(nz, df5, dt4, members, boxes, above, key0, thr, mask if with_mask else None, counts)
    assert got is counts
    torch.cuda.synchronize()
    return mask.cpu().numpy(), counts.cpu().numpy()


def plain_mask(df5, dt4, members, key0, thr_act, thr_inact):
    import torch
    from miniweatherml_amd import capi, modules
    nz, ncol, nens = df5[0].shape
    mask = torch.full((df5[0].numel(),), 7, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().mw_member_sample_mask(nz, ncol, nens, len(members), (C.c_int * len(members))(*members), modules._field_ptr_array(df5),
                                                modules._field_ptr_array(dt4), key0, thr_act, thr_inact, C.c_void_p(mask.data_ptr()), None))
    torch.cuda.synchronize()
    return mask.cpu().numpy()


# ---- 1. the kernel against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,members", cases())
def test_kernel_equals_the_numpy_statement(mw, shape, members):
    nz, ncol, nens = shape
    f5, t4 = base_state(nz, ncol, nens, seed=7 + nz * ncol)
    boxes = boxes_for(len(members))
    above = [j % 2 == 0 for j in range(len(members))]                          # mixed per member
    log = plant(f5, t4, members, boxes)
    assert log
    df5, dt4 = to_device(f5), to_device(t4)
    nelem = nz * ncol * nens
    thr = np.array([[0.9, 0.3, 0.1], [0.5, 1.0, 0.0], [0.0, 0.6, 0.7], [1.0, 0.2, 0.4]])[np.arange(len(members)) % 4]
    for seed in (1, 987654321):
        key0 = (seed * nelem) % 2 ** 64
        want_mask, want_counts = ref.mask_and_counts(f5, t4, members, boxes, above, key0, thr)
        mask, counts = device_call(df5, dt4, members, boxes, above, key0, thr)
        print(shape, members, "counts", counts.tolist())
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(mask, want_mask)
        listed = np.isin(np.arange(nelem) % nens, members)
        assert not mask[~listed].any()
        # a count-only call writes no mask byte, and its first three words are the mask call's
        mask2, counts2 = device_call(df5, dt4, members, boxes, above, key0, thr, with_mask=False, counts_fill=2 ** 40)
        assert (mask2 == 7).all() and np.array_equal(counts2, want_counts)
    if nelem >= 256:
        assert (want_counts[:, :3].sum(axis=0) > 0).all() and want_mask.any()  # every class is met at the shapes of more than one wavefront


def test_kernel_strides_over_more_elements_than_its_grid(mw):
    """The grid is capped at 4096 blocks of 256: 1,048,800 elements are one full stride and 224 elements of a second one (a block's
    tail), with six of eight members listed, so that a lane's member changes from one stride to the next."""
    nz, ncol, nens, members = 3, 43700, 8, [6, 1, 2, 3, 5, 4]
    assert 4096 * 256 < nz * ncol * nens < 4097 * 256 and (4096 * 256) % nens == 0
    f5, t4 = base_state(nz, ncol, nens, seed=11)
    boxes = boxes_for(len(members))
    above = [j % 2 == 1 for j in range(len(members))]
    plant(f5, t4, members, boxes)
    f5[0][nz - 1, ncol - 1, 5] = 1000.0                                        # outside, in the second stride
    thr = np.array([[0.9, 0.3, 0.1], [0.5, 1.0, 0.0], [0.0, 0.6, 0.7], [1.0, 0.2, 0.4], [1.0, 0.25, 0.25], [1.0, 1.0, 1.0]])
    key0 = (2 ** 64 - 5) % 2 ** 64                                             # the key wraps inside the fields
    want_mask, want_counts = ref.mask_and_counts(f5, t4, members, boxes, above, key0, thr)
    mask, counts = device_call(to_device(f5), to_device(t4), members, boxes, above, key0, thr)
    print("counts", counts.tolist())
    assert np.array_equal(counts, want_counts) and np.array_equal(mask, want_mask)
    assert want_mask[4096 * 256:].any() and want_mask[-3] == 1 and (want_counts[:, :3] > 0).all()


def planted_case():
    """One shape with every planted value at a column of its own, member 3 with `above` and member 1 without; the classes the reference
    gives are checked against the ones written down here.  Host only."""
    nz, ncol, nens, members, above = 4, 65, 4, [3, 1], [True, False]
    rng = np.random.default_rng(5)
    mid = np.array([275.0, 0.7, 0.005, 0.001, 0.002])
    f5 = [mid[v] * rng.uniform(0.99, 1.01, (nz, ncol, nens)) for v in range(5)]
    boxes = np.tile(BOX, (2, 1, 1))
    top = nz - 1
    plants = {0: (0, 0, BOX[0, 0]), 1: (0, top, BOX[0, 1]), 2: (0, 0, np.nextafter(BOX[0, 0], -np.inf)), 3: (2, top, np.nextafter(BOX[2, 1], np.inf)),
              4: (4, 0, -0.0), 5: (1, 2, 1.0e30), 6: (3, 1, np.nextafter(BOX[3, 1], np.inf)), 7: (0, top, BOX[0, 1]), 8: (0, 1, np.nan),
              10: (2, top, 1.0e300), 11: (1, 1, np.nan), 12: (4, 2, np.inf)}
    for c, (v, k, x) in plants.items():
        f5[v][k, c, :] = x
    t4 = [f5[v].copy() for v in BEFORE]                                        # the teacher leaves every element as it is: inactive ...
    t4[2][:, 20:, :] += 1.0e-6                                                 # ... but the columns from 20 on
    t4[2][2, 9, :] = np.inf
    t4[0][0, 13, :] = 1.0e300
    row, eligible, cls = ref.classify(f5, t4, members, boxes, above)
    cls = cls.reshape(nz, ncol, nens)
    for e, ab in ((3, True), (1, False)):
        assert cls[0, 0, e] == 2 and cls[top, 1, e] == 2                       # a value at a bound is inside
        assert cls[0, 2, e] == 0 and cls[top, 3, e] == 0                       # one beyond it is outside
        assert cls[0, 4, e] == 2 and cls[2, 5, e] == 2                         # -0.0 against lo = 0.0; 1e30 against an infinite bound
        assert cls[1, 6, e] == 0 and cls[0, 6, e] == (0 if ab else 2)          # the level above counts for a member with `above` alone
        assert cls[top, 7, e] == 2 and cls[top - 1, 7, e] == 2                 # at the top level `above` adds nothing
        assert cls[1, 8, e] == -1 and cls[0, 8, e] == -1 and cls[2, 8, e] == 2                          # a NaN input: its cell and the one below
        assert cls[2, 9, e] == -1 and cls[1, 9, e] == 2 and cls[0, 13, e] == -1                         # teacher values: their own cell only
        assert cls[top, 10, e] == -1 and cls[top - 1, 10, e] == -1             # finite in fp64, infinite in fp32
        assert cls[1, 11, e] == -1 and cls[0, 11, e] == 2                      # density_dry has no level above
        assert cls[2, 12, e] == -1 and cls[1, 12, e] == -1 and cls[3, 12, e] == 2
        assert cls[0, 30, e] == 1                                              # (an active element)
    assert (cls[:, :, [0, 2]] == -1).all()
    return f5, t4, members, boxes, above, cls


def test_planted_values_fall_where_the_header_says(mw):
    """The device gives the reference's mask and counts on planted_case, whose classes are the ones written down there."""
    f5, t4, members, boxes, above, cls = planted_case()
    nz, ncol, nens = f5[0].shape
    df5, dt4 = to_device(f5), to_device(t4)
    thr = np.array([[1.0, 0.0, 0.0], [1.0, 0.5, 0.25]])
    key0 = 99 * nz * ncol * nens
    mask, counts = device_call(df5, dt4, members, boxes, above, key0, thr)
    want_mask, want_counts = ref.mask_and_counts(f5, t4, members, boxes, above, key0, thr)
    assert np.array_equal(mask, want_mask) and np.array_equal(counts, want_counts)
    # with thr = (1, 0, 0) the mask is exactly the eligible outside cells; an ineligible cell is in no count
    m3 = mask.reshape(nz, ncol, nens)[:, :, 3]
    assert np.array_equal(m3 == 1, cls[:, :, 3] == 0) and counts[0, 3] == counts[0, 0] == int((cls[:, :, 3] == 0).sum()) and counts[0, 4] == counts[0, 5] == 0
    assert counts[:, :3].sum(axis=1).tolist() == [int((cls[:, :, e] >= 0).sum()) for e in (3, 1)]
    # nine cells hold a non-finite value or lie under one; columns 2, 3 and 6 are outside, for member 3 with the cells under 3 and 6 as well
    assert counts[0, :3].sum() == counts[1, :3].sum() == nz * ncol - 9 and counts[0, 0] == 5 and counts[1, 0] == 3


# ---- 2. the kernel against the plain mask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 257, 1), (5, 17, 3), (4, 65, 4)], ids=lambda s: "x".join(map(str, s)))
def test_with_an_unbounded_box_the_mask_is_the_plain_one(mw, shape):
    nz, ncol, nens = shape
    f5, t4 = base_state(nz, ncol, nens, seed=3)
    members = member_lists(nens)[-1]
    plant(f5, t4, members, boxes_for(len(members)))
    df5, dt4 = to_device(f5), to_device(t4)
    boxes = np.tile(INF_BOX, (len(members), 1, 1))
    key0 = 31 * nz * ncol * nens
    for ta, ti in ((0.3, 0.1), (1.0, 0.0), (0.0, 1.0)):
        thr = np.array([[0.77, ta, ti]] * len(members))
        mask, counts = device_call(df5, dt4, members, boxes, [True] * len(members), key0, thr)
        assert np.array_equal(mask, plain_mask(df5, dt4, members, key0, ta, ti))
        assert (counts[:, 0] == 0).all() and (counts[:, 3] == 0).all() and counts[:, 3:].sum() == int(mask.sum())


# ---- 3. the harvester -------------------------------------------------------------------------------------------------------------------------
def harvest_state(shape, seed):
    from test_gpu_surrogate_rollout import make_state
    return make_state(shape, seed=seed)


def narrow_boxes(state, members, share=0.9):
    """Per member the shipped scaling rows with temp's upper bound at the `share` quantile of the member's own temperatures."""
    from test_gpu_surrogate_rollout import nets
    from miniweatherml_amd import modules
    boxes = []
    for m in members:
        b = modules.domain_box([nets(5)[0]])
        b[0, 1] = np.quantile(state["temp"][..., m], share)
        boxes.append(b)
    return np.stack(boxes)


def harvester_on(state, directory, members, names, dt=1.0, **kw):
    from test_gpu_surrogate_rollout import load, make_coupler
    from miniweatherml_amd import modules
    c = make_coupler(*state["temp"].shape, modules.Microphysics_Kessler())
    load(c, state)
    h = modules.RolloutHarvester()
    os.makedirs(directory, exist_ok=True)
    h.init(c, names, members, str(directory), **kw)
    return h, c, h.harvest(c, dt, 0.0)


def test_harvester_takes_what_the_reference_takes(mw, tmp_path):
    from miniweatherml_amd import modules, surrogate_train as st
    shape = (13, 9, 9, 4)
    nz, ncol, nens = shape[0], shape[1] * shape[2], shape[3]
    state = harvest_state(shape, 41)
    members, names, above = [1, 3], ["a", "b"], [False, True]
    boxes = narrow_boxes(state, members)
    cfg = {"share": 0.25, "margin": 0.0, "fields": list(IN5)}
    h, c, added = harvester_on(state, tmp_path, members, names, samples_per_step=200, seed=5, outside=cfg, boxes=boxes, above=above)
    assert h.outside == cfg and h.last_counts.shape == (2, 6) and h.last_counts.dtype == np.int64
    f5 = [state[n].reshape(nz, ncol, nens) for n in IN5]
    t4 = [t.cpu().numpy().reshape(nz, ncol, nens) for t in h._teacher]
    ncell = nz * ncol
    thr = [ref.harvest_thresholds(200.0, 0.5, 0.4, ncell, 0.25, int(q)) for q in h.last_counts[:, 0]]    # the written formula on the call's own count
    assert np.array_equal(h.last_thresholds, np.array(thr))
    key0 = (5 * nz * ncol * nens) % 2 ** 64
    want_mask, want_counts = ref.mask_and_counts(f5, t4, members, boxes, above, key0, thr)
    print("counts", h.last_counts.tolist(), "thresholds", thr)
    assert np.array_equal(h.last_counts, want_counts) and np.array_equal(h.last_elems, np.flatnonzero(want_mask))
    assert (want_counts[:, 0] > 0.05 * ncell).all() and (want_counts[:, 3] > 0).all()                    # the premise: cells outside, and taken
    for j, (name, m) in enumerate(zip(names, members)):
        assert sum(h.taken[name].values()) == added[name] == int(want_counts[j, 3:].sum()) == st.read_samples([h.files[name]])[0].shape[0]
        assert h.taken[name] == dict(zip(modules.SAMPLE_CLASSES, want_counts[j, 3:].tolist()))
        assert h.eligible[name] == dict(zip(modules.SAMPLE_CLASSES, want_counts[j, :3].tolist()))
        for stencil in (False, True):
            ins, outs, _ = st.read_samples([h.files[name]], stencil=stencil)
            assert ins.shape == (added[name], 9 if stencil else 5) and outs.shape == (added[name], 4)
    first = {n: dict(h.taken[n]) for n in names}
    more = h.harvest(c, 1.0, 1.0)                                              # a second call: another draw, cumulative counts
    for j, name in enumerate(names):
        assert sum(h.taken[name].values()) == added[name] + more[name] == h.samples[name]
        assert h.taken[name]["outside"] == first[name]["outside"] + int(h.last_counts[j, 3])
        assert h.eligible[name]["outside"] == 2 * int(want_counts[j, 0])


def test_with_nothing_outside_the_harvest_is_the_plain_one_of_half_the_size(mw, tmp_path):
    """share 0.5 of 100 samples with a margin of 1e6 box widths: nothing is outside, `inside` is 50.0 exactly, and elements and files are those
    of a plain harvester that asks for 50."""
    from test_gpu_surrogate_rollout import nets
    from miniweatherml_amd import modules
    shape = (13, 9, 9, 4)
    state = harvest_state(shape, 43)
    boxes = np.stack([modules.domain_box([nets(5)[0]], margin=1.0e6)] * 2)
    cfg = {"share": 0.5, "margin": 1.0e6, "fields": list(IN5)}
    h, _, added = harvester_on(state, tmp_path / "outside", [1, 3], ["a", "b"], samples_per_step=100, seed=9, outside=cfg, boxes=boxes, above=[False, True])
    p, _, plain = harvester_on(state, tmp_path / "plain", [1, 3], ["a", "b"], samples_per_step=50, seed=9)
    assert p.outside is None and p.last_counts is None and not hasattr(p, "taken")
    assert added == plain and np.array_equal(h.last_elems, p.last_elems) and h.last_elems.size > 0
    assert (h.last_counts[:, 0] == 0).all() and (h.last_thresholds[:, 0] == 0.0).all()
    for name in ("a", "b"):
        assert open(h.files[name], "rb").read() == open(p.files[name], "rb").read()


def test_a_member_past_the_cap_is_left_out_of_both_calls(mw, tmp_path):
    from test_gpu_surrogate_rollout import make_state
    state = make_state((12, 3, 11, 3), seed=3, rain=False)
    state["precip_liquid"][..., 1] = 1.0e-2 * state["density_dry"][..., 1]
    boxes = narrow_boxes(state, [1, 2])
    cfg = {"share": 0.5, "margin": 0.0, "fields": list(IN5)}
    h, _, added = harvester_on(state, tmp_path, [1, 2], ["wet", "dry"], dt=300.0, samples_per_step=200, seed=2, max_rainsplit=4, outside=cfg,
                               boxes=boxes, above=[False, False])
    assert added["wet"] == 0 and h.skipped == {"wet": 1, "dry": 0} and added["dry"] > 0
    assert h.last_counts.shape == (1, 6) and not (h.last_elems % 3 == 1).any()
    assert h.taken["wet"] == h.eligible["wet"] == {"outside": 0, "active": 0, "inactive": 0}
    assert sum(h.taken["dry"].values()) == added["dry"] and h.taken["dry"]["outside"] > 0


def test_harvester_refusals(mw, tmp_path):
    from test_gpu_surrogate_rollout import make_coupler
    from miniweatherml_amd import modules
    c = make_coupler(4, 3, 3, 3, modules.Microphysics_Kessler())
    box = np.tile(BOX, (1, 1, 1))
    ok = {"share": 0.5, "margin": 0.0, "fields": list(IN5)}
    for kw in (dict(outside=ok), dict(outside=ok, boxes=box), dict(outside=ok, boxes=np.tile(BOX, (2, 1, 1)), above=[True]),
               dict(outside=dict(ok, share=0.0), boxes=box, above=[True]), dict(outside=dict(ok, share=True), boxes=box, above=[True]),
               dict(outside={"share": 0.5}, boxes=box, above=[True]), dict(boxes=box, above=[True])):
        with pytest.raises(modules.MWError, match="RolloutHarvester"):
            modules.RolloutHarvester().init(c, ["a"], [1], str(tmp_path), **kw)


# ---- 4. the rollout and the driver --------------------------------------------------------------------------------------------------------------
def has_key(doc, key):
    if isinstance(doc, dict):
        return key in doc or any(has_key(v, key) for v in doc.values())
    return isinstance(doc, list) and any(has_key(v, key) for v in doc)


def test_driver_harvests_outside_and_leaves_the_run_alone(mw, tmp_path, monkeypatch):
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from test_gpu_surrogate_rollout import ALL8, same
    from miniweatherml_amd import driver, surrogate_train as st
    entries, _ = write_models(tmp_path)
    entries = entries[:2]                                                       # one model of each width
    lst = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    monkeypatch.chdir(tmp_path)
    kw = dict(nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000.)
    path, _ = write_yaml(tmp_path, extra=lst + "harvest: {interval: 2, samples_per_step: 200, seed: 1, outside: {share: 0.5, margin: 0.0}}\n", **kw)
    c1, _, info = driver.run("rollout_surrogates", path, max_steps=4, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    hv = doc["harvest"]
    assert info["steps"] == 4 and hv["calls"] == 2 and hv["members"] == ["single_a", "stencil_a"]
    assert {k: hv["outside"][k] for k in ("share", "margin", "fields")} == {"share": 0.5, "margin": 0.0, "fields": list(IN5)}
    assert sorted(hv["outside"]["boxes"]) == ["single_a", "stencil_a"] and list(hv["outside"]["boxes"]["single_a"]) == list(IN5)
    for name in ("single_a", "stencil_a"):
        assert os.path.basename(hv["files"][name]) == "rollout_samples_%s.nc" % name and os.path.exists(hv["files"][name])
        assert list(hv["taken"][name]) == list(hv["eligible"][name]) == ["outside", "active", "inactive"]
        for cls in hv["taken"][name]:
            assert hv["eligible"][name][cls] >= hv["taken"][name][cls] >= 0
        assert sum(hv["taken"][name].values()) == hv["samples"][name] == st.read_samples([hv["files"][name]])[0].shape[0] > 0
        assert 0 < sum(hv["eligible"][name].values()) <= 2 * 10 * 12 * 16
    fields1 = {n: c1.get_data_manager_readonly().get(n, True).clone() for n in ALL8}
    # the run without a harvest block: every field of every member has the same bits, and the document no new key
    path, _ = write_yaml(tmp_path, extra=lst, **kw)
    c2, _, _ = driver.run("rollout_surrogates", path, max_steps=4, quiet=True)
    plain = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    for n in ALL8:
        assert same(fields1[n], c2.get_data_manager_readonly().get(n, True)), n
    assert "harvest" not in plain and plain["report"] == doc["report"] and plain["history"] == doc["history"]
    path, _ = write_yaml(tmp_path, extra=lst + "harvest: {interval: 2, samples_per_step: 200, seed: 1}\n", **kw)
    driver.run("rollout_surrogates", path, max_steps=4, quiet=True)
    old = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert sorted(old["harvest"]) == sorted(["interval", "samples_per_step", "ratio_active", "seed", "max_rainsplit", "members", "files", "samples",
                                             "skipped", "calls"])
    assert not any(has_key(old, k) for k in ("outside", "taken", "eligible", "nn_training_domain"))


# ---- 5. the table ---------------------------------------------------------------------------------------------------------------------------------
def test_training_domain_follows_the_training_sets_and_widens_a_rollout_s_box(mw, tmp_path):
    from test_gpu_surrogate_rollout import load, make_coupler
    from test_gpu_surrogate_train import kessler_like
    from test_surrogate_train_cpu import write_sample_file
    from miniweatherml_amd import driver, modules, surrogate_train as st
    sets = {}
    for name, seed in (("A", 2), ("B", 3), ("C", 4)):
        ins, outs = kessler_like(6000, seed)
        if name == "B":
            ins[:50, 0, :] *= 1.1                                              # temp up to 330 K
        if name == "C":
            ins[:50, 3, :] *= 2.0                                              # cloud_liquid up to 0.008
            ins[50:100, 0, :] = 190.0
        sets[name] = (write_sample_file(tmp_path / ("%s.nc" % name), [(ins, outs)]), ins[:, :, 0])
    d1, d2, d3 = (str(tmp_path / d) for d in ("first", "second", "third"))
    common = dict(epochs=1, batch_size=256, seed=4)
    r1 = st.train_surrogate([sets["A"][0]], d1, **common)
    r2 = st.train_surrogate([sets["A"][0], sets["B"][0]], d2, init=d1, keep_all=True, **common)
    r3 = st.train_surrogate([sets[k][0] for k in "ABC"], d3, init=d2, **common)
    scl_a = np.loadtxt(os.path.join(d1, "input_scaling.txt"))
    for d in (d2, d3):                                                         # the scaling rows stay A's
        assert np.array_equal(np.loadtxt(os.path.join(d, "input_scaling.txt")), scl_a)
    assert not os.path.exists(os.path.join(d1, "training_domain.txt")) and "training_domain" not in r1
    t2 = modules.load_training_domain(os.path.join(d2, "training_domain.txt"), 5)
    t3 = modules.load_training_domain(os.path.join(d3, "training_domain.txt"), 5)
    want2 = ref.domain_union(np.concatenate([sets["A"][1], sets["B"][1]]), scl_a)
    want3 = ref.domain_union(np.concatenate([sets[k][1] for k in "ABC"]), want2)
    assert np.array_equal(t2, want2) and np.array_equal(t3, want3) and np.array_equal(r2["training_domain"], want2)
    assert t2[0, 1] > scl_a[0, 1] and t3[0, 0] < t2[0, 0] and t3[3, 1] > t2[3, 1] and np.array_equal(t3[0, 1], t2[0, 1])
    # the second continuation starts from the first one's table: give it C alone and B's range is still there
    r4 = st.train_surrogate([sets["C"][0]], str(tmp_path / "fourth"), init=d2, **common)
    assert np.array_equal(r4["training_domain"], ref.domain_union(sets["C"][1], want2)) and r4["training_domain"][0, 1] == t2[0, 1] > scl_a[0, 1]
    assert r3["training_domain_file"] == os.path.join(d3, "training_domain.txt")
    assert all(m["nn_training_domain"] == r2["training_domain_file"] for m in r2["surrogate_models"]) and len(r2["surrogate_models"]) == 1
    # a rollout: one value between the old and the new upper bound of temp
    entry = {"name": "ft", "keras_weights_txt": os.path.join(d2, "weights.txt"), "nn_input_scaling": os.path.join(d2, "input_scaling.txt"),
             "nn_output_scaling": os.path.join(d2, "output_scaling.txt")}
    nz, ny, nx = 6, 5, 7
    rng = np.random.default_rng(8)
    state = {n: (scl_a[i, 0] + (scl_a[i, 1] - scl_a[i, 0]) * rng.uniform(0.1, 0.9, (nz, ny, nx, 2))) for i, n in enumerate(IN5)}
    for n in ("uvel", "vvel", "wvel"):
        state[n] = rng.uniform(-10.0, 10.0, (nz, ny, nx, 2))
    state["temp"][2, 3, 4, 1] = 0.5 * (scl_a[0, 1] + t2[0, 1])
    outside = {}
    for with_key in (True, False):
        entries = driver._surrogate_models([dict(entry, nn_training_domain=r2["training_domain_file"]) if with_key else dict(entry)], str(tmp_path))
        bank = modules.load_surrogate_bank(entries)
        micro = modules.Microphysics_Rollout()
        c = make_coupler(nz, ny, nx, 2, micro, models=bank, persistence=False, names=["ft"], domains=modules.load_training_domains(entries, bank))
        load(c, state)
        micro.training_domain, micro.domain_now = True, True
        micro.time_step(c, 1.0)
        micro.domain_record(0)
        block = micro.domain_reports()[1]
        outside[with_key] = (block["steps"][0]["outside_columns"], block["steps"][0]["above"]["temp"],
                             sum(sum(block["steps"][0][k].values()) for k in ("below", "above", "nan")), block["box"]["temp"])
    assert outside[True] == (0, 0, 0, [float(t2[0, 0]), float(t2[0, 1])])
    assert outside[False] == (1, 1, 1, [float(scl_a[0, 0]), float(scl_a[0, 1])])
