"""The training-domain guard on the GPU: mw_member_domain against the numpy statement of domain_ref, its set / add
contract and refusals; the guarded step with a box against the unguarded committee (a box nothing leaves), the members teacher (a box
nothing satisfies) and the step composed from the entry points that existed before; the rollout's guard and report; the driver's
document; the inference path.

Everything is integer or bitwise: "equal" is == on counts and the same bits on fields (test_gpu_surrogate_rollout.same).  Every case is
a few thousand cells."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import domain_ref
from test_domain_guard_cpu import call_domain, refusal_cases
from test_gpu_committee_guard import DZ, OWN, SENTINEL, columns_teacher, gpu, host_flags, lib, member_state, ptrs, stream
from test_gpu_surrogate_rollout import ALL8, IN5, OUT4, make_state, same

pytestmark = pytest.mark.gpu


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def boxes_for(nm):
    """A different box per listed member; the draws of [0, 1) are inside all of them.  precip_liquid's lo is 0.0 (for -0.0), and the
    second member's water_vapor is unbounded (for +-inf against an infinite bound)."""
    b = np.empty((nm, 5, 2))
    for j in range(nm):
        for f in range(5):
            b[j, f] = (-(0.5 + j + f / 8.0), 1.5 + j + f / 8.0)
        b[j, 4, 0] = 0.0
    if nm > 1:
        b[1, 2] = (-math.inf, math.inf)
    return b


def planted_state(nz, ncol, nens, members, boxes, seed):
    """Five host fields (nz, ncol, nens) in [0, 1) with, for every listed member, values exactly at lo and at hi (inside), nextafter
    beyond each, NaN, +inf and -inf, and -0.0 against lo = 0, at level 0, level nz - 1 and in between; the unlisted members hold NaN."""
    rng = np.random.default_rng(seed)
    x = [rng.uniform(0.0, 1.0, (nz, ncol, nens)) for _ in range(5)]
    top, mid = nz - 1, nz // 2
    a, b, c, d, e_, f_ = 0, ncol - 1, ncol // 2, ncol // 3, (2 * ncol) // 3, min(1, ncol - 1)
    for e in range(nens):
        if e not in members:
            for f in range(5):
                x[f][..., e] = math.nan
    for j, e in enumerate(members):
        lo, hi = boxes[j, :, 0], boxes[j, :, 1]
        x[0][0, a, e] = lo[0]                                                   # at lo, at hi, -0.0 at lo = 0.0: inside
        x[1][top, a, e] = hi[1]
        x[4][0, a, e] = -0.0
        x[4][mid, d, e] = 0.0
        x[0][0, b, e] = np.nextafter(lo[0], -math.inf)                          # one step beyond each
        x[1][top, c, e] = np.nextafter(hi[1], math.inf)
        x[4][top, c, e] = -5e-324                                               # the smallest negative number against lo = 0.0
        x[3][mid, d, e] = math.nan
        x[3][top, e_, e] = math.inf
        x[3][0, f_, e] = -math.inf
        x[2][mid, e_, e] = math.inf                                             # against [-inf, inf] for the second member: inside
        x[2][0, f_, e] = -math.inf
        x[2][top, b, e] = math.nan                                              # NaN is outside every box
    return x


def run_domain(dx, members, boxes, counts, flags=None, slots=None, flag_counts=None):
    from miniweatherml_amd import capi
    nz, ncol, nens = dx[0].shape
    capi.check(lib().mw_member_domain(nz, ncol, nens, len(members), (C.c_int * len(members))(*members),
                                      np.ascontiguousarray(boxes).ctypes.data_as(C.POINTER(C.c_double)), ptrs(dx), C.c_void_p(counts.data_ptr()),
                                      None if flags is None else C.c_void_p(flags.data_ptr()),
                                      None if slots is None else (C.c_int * len(slots))(*slots),
                                      None if flag_counts is None else C.c_void_p(flag_counts.data_ptr()), stream()))


@pytest.mark.parametrize("nens,members", [(1, [0]), (3, [1]), (4, [3, 1])])
@pytest.mark.parametrize("ncol", [1, 63, 65, 130])
@pytest.mark.parametrize("nz", [1, 2, 5, 9, 17])
def test_kernel_against_numpy(mw, nz, ncol, nens, members):
    import torch
    boxes = boxes_for(len(members))
    x = planted_state(nz, ncol, nens, members, boxes, seed=1000 * nz + 10 * ncol + nens)
    dx = [gpu(a) for a in x]
    want = domain_ref.classify(x, members, boxes)
    if ncol >= 6:                                                               # the planted cells, in the numpy statement itself
        for j in range(len(members)):
            inf_inside = j == 1
            assert want[j, 0] == 1 and want[j, 4] == 1 and want[j, 12] == 1 and want[j, 11] == 1 and want[j, 8] == 1, want[j]
            assert want[j, 9] == 1 and want[j, 10] == 1 and want[j, 15] == 5
            assert want[j, 6] == (0 if inf_inside else 1) and want[j, 7] == (0 if inf_inside else 1)
            assert want[j, 1] == want[j, 2] == want[j, 3] == want[j, 5] == want[j, 13] == want[j, 14] == 0
    counts = torch.full((len(members), 16), -77, dtype=torch.int64, device="cuda")
    run_domain(dx, members, boxes, counts)                                      # report only: no flags
    assert np.array_equal(counts.cpu().numpy(), want), (counts.cpu().numpy(), want)
    for slots in ([[0]] if len(members) == 1 else [[1, -1], [0, 1], [-1, -1]]):
        flags0 = np.zeros((ncol, nens), dtype=np.uint8)
        for j, e in enumerate(members):
            if slots[j] >= 0:
                flags0[[ncol - 1, ncol // 2], e] = 1                            # preset on columns that are outside too
            else:
                flags0[:, e] = 7
        for e in range(nens):
            if e not in members:
                flags0[:, e] = 7
        fc0 = np.array([[5, 9], [11, 13]], dtype=np.int64)
        wc, wflags, wfc = domain_ref.classify(x, members, boxes, flags0, slots, fc0)
        flags, fc = gpu(flags0), gpu(fc0)
        counts.fill_(-77)
        run_domain(dx, members, boxes, counts, flags, slots, fc)
        got = flags.cpu().numpy()
        assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(wc, want)
        assert np.array_equal(got, wflags), (slots, np.nonzero(got != wflags))
        for j, e in enumerate(members):
            if slots[j] < 0:
                assert (got[:, e] == 7).all()
            else:
                assert (got[[ncol - 1, ncol // 2], e] == 1).all()
                newly = int(((got[:, e] == 1) & (flags0[:, e] == 0)).sum())
                assert newly == want[j, 15] - len({ncol - 1, ncol // 2})        # the preset bytes are not counted
                assert fc.cpu().numpy()[slots[j]].tolist() == [fc0[slots[j], 0] + newly, fc0[slots[j], 1] + newly]
        for e in range(nens):
            if e not in members:
                assert (got[:, e] == 7).all()
        assert np.array_equal(fc.cpu().numpy(), wfc)
        run_domain(dx, members, boxes, counts, flags, slots, fc)                # counts is SET again, flag_counts adds 0
        assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(fc.cpu().numpy(), wfc) and np.array_equal(flags.cpu().numpy(), wflags)
    for t, a in zip(dx, x):
        assert same(t, gpu(a))                                                  # the fields are only read


def test_python_entry_and_more_than_one_block_per_member(mw):
    """modules.member_domain on a (nz, ny, nx, nens) state with six of eight members listed, against the numpy statement."""
    import torch
    from miniweatherml_amd import modules
    nz, ny, nx, nens = 11, 7, 19, 8
    members = [6, 1, 2, 7, 4, 3]
    boxes = np.stack([np.stack([np.full(5, 0.05 * j), np.full(5, 1.0 - 0.03 * j)], axis=1) for j in range(6)])
    rng = np.random.default_rng(8)
    x = [rng.uniform(0.0, 1.0, (nz, ny * nx, nens)) for _ in range(5)]
    want = domain_ref.classify(x, members, boxes)
    assert (want[1:, :15:3] > 0).all() and (want[1:, 1:15:3] > 0).all() and not want[0].any() and 0 < want[1, 15] <= ny * nx
    dx = [gpu(a).reshape(nz, ny, nx, nens) for a in x]
    counts = modules.member_domain(nz, dx, members, boxes)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (6, 16) and np.array_equal(counts.cpu().numpy(), want)
    again = modules.member_domain(nz, dx, members, boxes, counts)
    assert again is counts and np.array_equal(counts.cpu().numpy(), want)
    g = modules.CommitteeGuard(dx[0], nz, slots=2)
    slots = [-1, 1, -1, -1, 0, -1]
    modules.member_domain(nz, dx, members, boxes, counts, g, slots)
    wc, wflags, wfc = domain_ref.classify(x, members, boxes, np.zeros((ny * nx, nens), np.uint8), slots, np.zeros((2, 2), np.int64))
    assert np.array_equal(g.flags.cpu().numpy().reshape(ny * nx, nens), wflags) and np.array_equal(g.counts.cpu().numpy(), wfc)
    assert g.flagged_members == {1, 4}
    with pytest.raises(modules.MWError, match="one slot per member"):
        modules.member_domain(nz, dx, members, boxes, counts, g, [0])
    with pytest.raises(modules.MWError, match="box for each"):
        modules.member_domain(nz, dx, members, boxes[:5])


def test_refusals_write_nothing(mw):
    import torch
    L = lib()
    nz, ncol, nens = 4, 16, 3
    dx = [torch.zeros((nz, ncol, nens), dtype=torch.float64, device="cuda") for _ in range(5)]
    counts = torch.full((33, 16), -77, dtype=torch.int64, device="cuda")
    flags = torch.full((ncol, 64), 7, dtype=torch.uint8, device="cuda")
    fc = torch.full((2, 2), -5, dtype=torch.int64, device="cuda")
    for kw, msg in refusal_cases():
        rc = call_domain(L, [t.data_ptr() for t in dx], counts.data_ptr(), flags.data_ptr(), fc.data_ptr(), **kw)
        assert rc != 0 and msg in L.mw_last_error(), kw
        torch.cuda.synchronize()
        assert bool((counts == -77).all()) and bool((flags == 7).all()) and bool((fc == -5).all()), kw
    assert call_domain(L, [t.data_ptr() for t in dx], counts.data_ptr(), flags.data_ptr(), fc.data_ptr(), slots=[0, 1]) == 0     # the valid call
    assert counts[:2].cpu().tolist() == [[0] * 16] * 2 and bool((counts[2:] == -77).all())


# ---- 2. the guarded step ------------------------------------------------------------------------------------------------------------------
def guarded_step(bk, sel, member, f5, thr4, dt, box, cap=64):
    from miniweatherml_amd import modules
    state = [t.clone() for t in f5]
    g = modules.CommitteeGuard(state[0], state[0].shape[0])
    bk.committee_guard_apply(state[0].shape[0], sel, member, state, thr4, cap, DZ, dt, g, domain_box=box)
    return state, g


def composed_step(bk, sel, member, f5, host5, thr4, dt, box):
    """The step from the entry points that existed before: committee_apply out of place; the range's flags R and the box's flags D in
    numpy; mw_kessler_columns_teacher with the host-made flags of R | D; torch.where by those flags.  -> (the five fields after the
    step, R, D)."""
    import torch
    nz, ncol, nens = f5[0].shape
    mean = [torch.full_like(f5[0], SENTINEL) for _ in range(4)]
    rnge = [torch.full_like(f5[0], SENTINEL) for _ in range(4)]
    bk.committee_apply(nz, sel, member, f5, mean, rnge)
    R = host_flags([m[..., member].cpu().numpy() for m in mean], [r[..., member].cpu().numpy() for r in rnge], thr4)
    _, dflags, _ = domain_ref.classify(host5, [member], [box], np.zeros((ncol, nens), np.uint8), [0], np.zeros((1, 2), np.int64))
    D = dflags[:, member].astype(bool)
    flags = np.zeros((ncol, nens), bool)
    flags[:, member] = R | D
    kes, rs, _ = columns_teacher(f5, flags, dt)
    assert rs[member] == 1
    pick = gpu(flags[:, member]).reshape(1, ncol)
    after = [t.clone() for t in f5]
    for v, m, k in zip(OWN, mean, kes):
        after[v][..., member] = torch.where(pick, k[..., member], m[..., member])
    return after, R, D


@pytest.mark.parametrize("nens,member", [(1, 0), (4, 2)])
@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in", [5, 9])
def test_guarded_step_with_a_box(mw, n_in, strict, nens, member):
    import torch
    from test_gpu_surrogate_committee import SELS, bank, nets
    from miniweatherml_amd import capi, modules
    nz, ncol, dt = 8, 70, 1.0
    bk = bank(n_in)
    bk.strict = strict
    sel = SELS[3]
    models = [nets(n_in)[i] for i in sel]
    host = member_state(nz, ncol, nens, seed=n_in + 7 * nens)
    f5 = [gpu(a) for a in host]
    inf4 = (math.inf,) * 4
    # a wide box, no threshold: the unguarded committee in place
    plain = [t.clone() for t in f5]
    bk.committee_apply(nz, sel, member, plain, [plain[v] for v in OWN])
    assert all(bool(torch.isfinite(t).all()) for t in plain)
    got, g = guarded_step(bk, sel, member, f5, inf4, dt, modules.domain_box(models, 1.0e6))
    assert g.read(dt, [member])[0] == [(0, 0)] and g.domain_counts.cpu().tolist() == [[0] * 16]
    for n, a, b in zip(IN5, got, plain):
        assert same(a, b), n
    # a box no cell satisfies: the members teacher on that member
    narrow = np.array([[0.0, 1.0]] + [[-math.inf, math.inf]] * 4)
    got, g = guarded_step(bk, sel, member, f5, inf4, dt, narrow)
    assert g.read(dt, [member])[0] == [(ncol, ncol)]
    words = g.domain_counts.cpu().tolist()[0]
    assert words[1] == nz * ncol and words[15] == ncol and sum(words) == nz * ncol + ncol
    teach = [t.clone() for t in f5]
    ws = torch.empty(lib().mw_kessler_members_teacher_workspace_bytes(nz, ncol, nens) // 8, dtype=torch.float64, device="cuda")
    capi.check(lib().mw_kessler_members_teacher(nz, ncol, nens, 1, (C.c_int * 1)(member), DZ, dt, 64, ptrs(f5), ptrs([teach[v] for v in OWN]),
                                                None, C.c_void_p(ws.data_ptr()), stream()))
    for n, a, b in zip(IN5, got, teach):
        assert same(a, b), n
    # the partial case: D planted outside the box, R from the range; the flagged columns are R | D and the step is the composed form
    box = modules.domain_box(models, 0.25)
    assert np.array_equal(box, domain_ref.box_of([m[4] for m in models], 0.25))
    D = np.zeros(ncol, bool)
    D[[0, 17, 40, 64, 69]] = True
    host = [a.copy() for a in host]
    host[0][0, 0, member] = np.nextafter(box[0, 1], math.inf)                  # level 0, one step above
    host[2][nz - 1, 17, member] = np.nextafter(box[2, 0], -math.inf)           # the top level, one step below
    host[3][3, 40, member] = box[3, 1] * 1.5
    host[1][5, 64, member] = box[1, 1] * 1.01                                   # density_dry, which no network writes
    host[4][nz - 1, 69, member] = box[4, 1] * 2.0
    host[0][2, 30, member] = box[0, 1]                                          # exactly at the bound: inside
    f5 = [gpu(a) for a in host]
    rnge = [torch.empty_like(f5[0]) for _ in range(4)]
    bk.committee_apply(nz, sel, member, f5, [torch.empty_like(f5[0]) for _ in range(4)], rnge)
    col_max = rnge[0][..., member].cpu().numpy().max(axis=0)
    thr4 = (float(np.quantile(col_max, 0.75, method="lower")), math.inf, math.inf, math.inf)
    want, R, Dref = composed_step(bk, sel, member, f5, host, thr4, dt, box)
    assert np.array_equal(Dref, D) and 0 < R.sum() < ncol and (R & ~D).any() and (D & ~R).any()
    got, g = guarded_step(bk, sel, member, f5, thr4, dt, box)
    assert np.array_equal(g.flags.cpu().numpy().reshape(ncol, nens)[:, member].astype(bool), R | D)
    n = int((R | D).sum())
    assert g.read(dt, [member]) == ([(n, n)], [1])
    assert g.domain_counts.cpu().tolist()[0][15] == int(D.sum())
    for name, a, b in zip(IN5, got, want):
        assert same(a, b), name
    if nens > 1:
        others = [e for e in range(nens) if e != member]
        assert not g.flags.cpu().numpy().reshape(ncol, nens)[:, others].any()


# ---- 3. the rollout -----------------------------------------------------------------------------------------------------------------------
def test_rollout_with_a_domain_guarded_committee_of_one_beside_its_twin(mw):
    """Members: Kessler, the model, the committee of that one model, the same committee with guard {domain: margin 1e6} -- a box nothing
    leaves -- and persistence.  The twins start from one state and stay bitwise equal; the guard's record shows no flagged column."""
    from test_gpu_surrogate_rollout import fields, load, make_coupler, model_list
    from miniweatherml_amd import modules
    nz, ny, nx = 8, 12, 12
    models, names = model_list("single", 1), ["a"]
    state = make_state((nz, ny, nx, 5), seed=21)
    for n in state:
        state[n][..., 3] = state[n][..., 2]
    micro = modules.Microphysics_Rollout()
    c = make_coupler(nz, ny, nx, 5, micro, models=models, persistence=True, names=names,
                     committees=[("twin", names), ("boxed", names, {"domain": {"margin": 1.0e6}})])
    assert micro.member_names == ["kessler", "a", "twin", "boxed", "persistence"]
    load(c, state)
    for step in range(3):
        micro.time_step(c, 1.0)
        micro.guard_record(step, 1.0)
        got = fields(c)
        for n in ALL8:
            assert same(got[n][..., 3], got[n][..., 2]), (n, step)
    g = micro.guard_reports()[1]
    assert micro.guard_reports()[0] is None
    assert set(g) == {"thresholds", "max_rainsplit", "columns", "flagged_total", "steps", "domain"}
    assert g["thresholds"] == {f: "inf" for f in OUT4} and g["flagged_total"] == 0
    assert g["domain"]["margin"] == 1.0e6 and g["domain"]["fields"] == list(IN5) and set(g["domain"]["box"]) == set(IN5)
    assert g["steps"] == [{"step": s, "flagged": 0, "rainsplit": 1, "outside_columns": 0} for s in range(3)]
    json.dumps(g, allow_nan=False)


def test_rollout_guard_hands_outside_columns_to_kessler(mw):
    """The same members with margin 0 and a few columns of the twins planted outside the box: after one step the guarded member differs
    from its twin in exactly those columns, where it holds Kessler's bits (the members teacher's); flagged and outside_columns say so."""
    from test_gpu_surrogate_rollout import fields, load, make_coupler, model_list
    from miniweatherml_amd import modules
    nz, ny, nx = 8, 12, 12
    models, names = model_list("single", 1), ["a"]
    box = modules.domain_box(models)
    state = make_state((nz, ny, nx, 5), seed=22)
    cols = [(0, 0), (5, 7), (11, 11)]
    for j, i in cols:
        state["temp"][nz - 1, j, i, 2] = box[0, 1] + 1.0
    for n in state:
        state[n][..., 3] = state[n][..., 2]
    micro = modules.Microphysics_Rollout()
    c = make_coupler(nz, ny, nx, 5, micro, models=models, persistence=True, names=names, committees=[("twin", names), ("boxed", names, {"domain": True})])
    load(c, state)
    teach = modules.kessler_members_teacher(c, [3], 1.0)
    teach = [t.clone() for t in teach]
    micro.time_step(c, 1.0)
    micro.guard_record(0, 1.0)
    got = fields(c)
    differs = np.zeros((ny, nx), bool)
    for n in OUT4:
        a, b = got[n][..., 3].cpu().numpy(), got[n][..., 2].cpu().numpy()
        differs |= (a.view(np.int64) != b.view(np.int64)).any(axis=0)
    want = np.zeros((ny, nx), bool)
    for j, i in cols:
        want[j, i] = True
    assert np.array_equal(differs, want)
    for n, t in zip(OUT4, teach):
        for j, i in cols:
            assert same(got[n][:, j, i, 3], t[:, j, i, 3]), (n, j, i)
    s = micro.guard_reports()[1]["steps"]
    assert s == [{"step": 0, "flagged": 3, "rainsplit": 1, "outside_columns": 3}]
    assert not micro._guard.flags.cpu().numpy().reshape(ny * nx, 5)[:, [0, 1, 2, 4]].any()
    assert micro._guard_domain_counts.cpu().tolist() == [[0, 3] + [0] * 13 + [3]]                       # three temp cells above, three columns


def test_training_domain_only_reads_and_records_what_numpy_counts(mw):
    """Kessler, a single-cell and a stencil model, the committee of the single-cell one, persistence; a few planted outside values.  With
    training_domain on, every field of every member equals the run without it, and each step's record equals domain_ref on a copy of
    the state taken before the step (the report's place is before members_apply, and nothing before it writes a network-stepped member)."""
    from test_gpu_surrogate_rollout import fields, load, make_coupler, model_list
    from miniweatherml_amd import modules
    nz, ny, nx = 8, 12, 12
    models, names = model_list("mixed", 2), ["s9", "s5"]
    state = make_state((nz, ny, nx, 5), seed=23)
    state["temp"][0, 3, 4, 1] *= 2.0
    state["water_vapor"][nz - 1, 11, 0, 2] = -1.0
    state["cloud_liquid"][4, 6, 6, 3] = math.nan
    runs = {}
    for on in (False, True):
        micro = modules.Microphysics_Rollout()
        c = make_coupler(nz, ny, nx, 5, micro, models=models, persistence=True, names=names, committees=[("c5", ["s5"])])
        load(c, state)
        if on:
            micro.training_domain = {"margin": 0.0}
        wants = []
        for step in range(3):
            before = fields(c, IN5)
            micro.domain_now = on and step != 1                                 # no pass at step 1: nothing is recorded for it
            micro.time_step(c, 1.0)
            micro.domain_record(step)
            if on and step != 1:
                boxes = [modules.domain_box([models[0]]), modules.domain_box([models[1]]), modules.domain_box([models[1]])]
                host = [before[n].cpu().numpy().reshape(nz, ny * nx, 5) for n in IN5]
                wants.append((step, domain_ref.classify(host, [1, 2, 3], boxes)))
        runs[on] = fields(c)
        if on:
            assert [s for s, _ in micro._domain_steps] == [0, 2]
            for (s, got), (ws, want) in zip(micro._domain_steps, wants):
                assert s == ws and np.array_equal(got, want), (s, got, want)
            assert wants[0][1][0, 1] >= 1 and wants[0][1][1, 6] >= 1 and wants[0][1][2, 11] == 1 and (wants[0][1][:, 15] >= 1).all()
            rep = micro.domain_reports()
            assert rep[0] is None and rep[4] is None and all(rep[m]["cells"] == nz * ny * nx and rep[m]["columns"] == ny * nx for m in (1, 2, 3))
            assert [s["step"] for s in rep[1]["steps"]] == [0, 2] and rep[1]["first_outside_step"] == 0
            assert rep[3]["steps"][0]["nan"]["cloud_liquid"] == 1 and rep[3]["steps"][0]["outside_columns"] == int(wants[0][1][2, 15])
            json.dumps(rep, allow_nan=False)
    for n in ALL8 + ("precl",):
        assert same(runs[True][n], runs[False][n]), n


# ---- 4. the driver and the inference path -------------------------------------------------------------------------------------------------
def has_key(doc, key):
    if isinstance(doc, dict):
        return key in doc or any(has_key(v, key) for v in doc.values())
    return isinstance(doc, list) and any(has_key(v, key) for v in doc)


def test_driver_rollout_with_training_domain_and_a_domain_guard(mw, tmp_path, monkeypatch):
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from miniweatherml_amd import driver
    entries, _ = write_models(tmp_path)                                         # single_a, stencil_a, single_b
    text = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    text += "eval_interval: 2\nsurrogate_committees:\n  - {name: plain, members: [single_b, single_a]}\n"
    twin = "  - {name: boxed, members: [single_a]}\n"
    new = "  - {name: boxed, members: [single_a], guard: {domain: {margin: 0.0}}}\ntraining_domain: true\n"
    monkeypatch.chdir(tmp_path)
    nz, ny, nx = 10, 12, 16
    path, _ = write_yaml(tmp_path, nens=7, nx=nx, ny=ny, nz=nz, xlen=8000., ylen=6000., extra=text + new)
    c1, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert doc["members"] == ["kessler", "single_a", "stencil_a", "single_b", "plain", "boxed", "persistence"]
    blocks = [m["domain"] for m in doc["models"]] + [c["domain"] for c in doc["committees"]]
    assert len(blocks) == 5 and sorted(info["domain_reports"]) == sorted(doc["members"][1:6])
    for b in blocks:
        assert list(b) == ["margin", "fields", "box", "cells", "columns", "first_outside_step", "steps"]
        assert b["margin"] == 0.0 and b["fields"] == list(IN5) and list(b["box"]) == list(IN5) and all(len(v) == 2 for v in b["box"].values())
        assert b["cells"] == nz * ny * nx and b["columns"] == ny * nx
        assert [s["step"] for s in b["steps"]] == [0, 2]
        for s in b["steps"]:
            assert list(s) == ["step", "outside_columns", "below", "above", "nan"] and 0 <= s["outside_columns"] <= ny * nx
            assert all(list(s[k]) == list(IN5) and all(0 <= v <= b["cells"] for v in s[k].values()) for k in ("below", "above", "nan"))
        hit = [s["step"] for s in b["steps"] if s["outside_columns"] > 0]
        assert b["first_outside_step"] == (hit[0] if hit else None)
    assert "guard" not in doc["committees"][0]
    g = doc["committees"][1]["guard"]
    assert g["thresholds"] == {f: "inf" for f in OUT4} and g["columns"] == ny * nx
    assert g["domain"] == {"margin": 0.0, "fields": list(IN5), "box": doc["committees"][1]["domain"]["box"]}
    assert [s["step"] for s in g["steps"]] == [0, 2]
    for s, r in zip(g["steps"], doc["committees"][1]["domain"]["steps"]):
        # no threshold: the union is the box's columns, and the report saw the same state with the same box
        assert list(s) == ["step", "flagged", "rainsplit", "outside_columns"] and s["flagged"] == s["outside_columns"] == r["outside_columns"]
    path, _ = write_yaml(tmp_path, nens=7, nx=nx, ny=ny, nz=nz, xlen=8000., ylen=6000., extra=text + twin)
    driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert not has_key(doc, "domain") and not has_key(doc, "outside_columns")


def test_inference_path_with_a_domain_guard(mw):
    """Microphysics_Kessler_Surrogate with a committee of one and guard {domain: true}: what it returns is committee_guard_apply with the
    model's box on the state before the call (all members' columns as one member)."""
    from test_gpu_surrogate_committee import nets as nets16
    from test_gpu_surrogate_rollout import load, make_coupler
    from miniweatherml_amd import modules
    nz, ny, nx, nens = 8, 3, 10, 2
    m = nets16(5)[2]
    box = modules.domain_box([m])
    state = make_state((nz, ny, nx, nens), seed=5)
    state["temp"][2, 1, 4, 1] = box[0, 1] * 1.25
    state["precip_liquid"][nz - 1, 2, 9, 0] = box[4, 1] * 1.5
    bk = modules.SurrogateBank([m])
    f5 = [gpu(state[n]).reshape(nz, -1, 1) for n in IN5]
    want, g = guarded_step(bk, [0], 0, f5, (math.inf,) * 4, 1.0, box)
    assert g.read(1.0)[0] == [(2, 2)]
    micro = modules.Microphysics_Kessler_Surrogate()
    c = make_coupler(nz, ny, nx, nens, micro, committee=[m], guard={"domain": True})
    load(c, state)
    out = micro.time_step(c, 1.0)
    for v, n in zip(OWN, OUT4):
        assert same(out[OUT4.index(n)].reshape(nz, -1, 1), want[v]), n
    assert micro._guard.read(1.0)[0] == [(2, 2)]
