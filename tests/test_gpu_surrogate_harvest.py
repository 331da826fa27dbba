"""Harvesting Kessler labels on the rollout members' own states, on the GPU: the teacher (mw_kessler_members_teacher) against the
production Kessler on each member alone, bit for bit; its per-member sub-cycle count, its bound and a diverged member; the member-layout
sample mask and gather against their numpy statement; RolloutHarvester's files; the rollout step and the rollout_surrogates experiment
with and without a harvester; the trainer's warm start.

"Equal" is the same bits throughout (test_gpu_surrogate_rollout.same)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_surrogate_rollout import ALL8, IN5, OUT4, fields, kessler_alone, load, make_coupler, make_state, nets, same
from test_surrogate_harvest_cpu import u01

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 15, 3), (9, 1, 1, 4), (22, 3, 11, 5), (13, 9, 9, 4), (37, 25, 40, 3)]
SENTINEL = -777.25
DT = 1.0


def teacher(state, members, dt=DT, cap=64):
    """mw_kessler_members_teacher through modules.kessler_members_teacher on a coupler that holds the state, the four outputs pre-filled
    with a sentinel: (outputs, counts, the coupler's five fields after the call)."""
    import torch
    from miniweatherml_amd import modules
    shape = state["temp"].shape
    c = make_coupler(*shape, modules.Microphysics_Kessler())
    load(c, state)
    outs = [torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda") for _ in range(4)]
    got, rs = modules.kessler_members_teacher(c, members, dt, cap, outs, return_rainsplit=True)
    assert all(a is b for a, b in zip(got, outs))
    return outs, rs, fields(c, IN5)


def is_sentinel(t):
    return bool((t == SENTINEL).all())


def device(state, names=IN5):
    import torch
    return {n: torch.from_numpy(np.ascontiguousarray(state[n])).cuda() for n in names}


# ---- 1. the teacher equals Kessler alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_teacher_equals_kessler_alone(mw, shape):
    """Member lists "all but 0", one member, and a pair that is not contiguous (0 and the last).  The reference is the production Kessler
    (strict = 0) on a nens = 1 coupler that holds the member."""
    nens = shape[3]
    state = make_state(shape, seed=sum(shape))
    before = device(state)
    alone, counts = zip(*[kessler_alone(state, m, 0, return_rainsplit=True) for m in range(nens)])
    for members in (list(range(1, nens)), [nens - 2], [nens - 1, 0]):
        outs, rs, after = teacher(state, members)
        assert rs == [counts[m] for m in members]
        for n in IN5:
            assert same(after[n], before[n]), (n, "the coupler's field was written")
        for m in range(nens):
            for n, o in zip(OUT4, outs):
                if m in members:
                    assert same(o[..., m], alone[m][n][..., 0]), (n, m, members)
                else:
                    assert is_sentinel(o[..., m]), (n, m, members)


# ---- 2. per-member sub-cycling and its bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 3, 11, 3), (7, 9, 31, 3)], ids=lambda s: "x".join(map(str, s)))
def test_every_member_has_its_own_count(mw, shape):
    """99 columns (one workgroup of the sub-cycling sweep) and 837 (four, the last one partial).  The premise below holds at any shape: dz
    is 500 m whatever nz is, member 1's rain of 1e-2 rho_d falls at 7 .. 27 m/s over the shipped density range, and 300 s of that against
    0.8 dz are 6 .. 21 sub-cycles."""
    dt = 300.0
    state = make_state(shape, seed=3, rain=False)
    state["precip_liquid"][..., 1] = 1.0e-2 * state["density_dry"][..., 1]
    a1, c1 = kessler_alone(state, 1, 0, dt, return_rainsplit=True)
    a2, c2 = kessler_alone(state, 2, 0, dt, return_rainsplit=True)
    print("alone: member 1 sub-cycles %d times, member 2 %d" % (c1, c2))
    assert c1 > 4 and c1 <= 64 and c2 == 1                                    # the premise (and that the cap of 4 below bites)
    outs, rs, _ = teacher(state, [1, 2], dt, 64)
    assert rs == [c1, 1]
    for n, o in zip(OUT4, outs):
        assert same(o[..., 1], a1[n][..., 0]) and same(o[..., 2], a2[n][..., 0]), n
        assert is_sentinel(o[..., 0]), n
    capped, rs, _ = teacher(state, [1, 2], dt, 4)
    assert rs == [0, 1]
    for n, o, full in zip(OUT4, capped, outs):
        assert is_sentinel(o[..., 1]) and is_sentinel(o[..., 0]), n
        assert same(o[..., 2], full[..., 2]), n


# ---- 3. a diverged member --------------------------------------------------------------------------------------------------------------
def test_a_diverged_member_stays_in_its_lane(mw):
    """One inf in member 1's rain (its rain CFL step is 0: skipped), one NaN in member 2's temperature (whatever its own cells become);
    members 0 and 3 are finite and equal their alone results."""
    shape = (9, 2, 3, 4)
    state = make_state(shape, seed=21)
    state["precip_liquid"][4, 1, 2, 1] = np.inf
    state["temp"][6, 0, 1, 2] = np.nan
    outs, rs, _ = teacher(state, [0, 1, 2, 3])
    assert rs[1] == 0 and rs[0] == 1 and rs[3] == 1
    for m in (0, 3):
        want = kessler_alone(state, m, 0)[0]
        for n, o in zip(OUT4, outs):
            assert same(o[..., m], want[n][..., 0]), (n, m)
    for n, o in zip(OUT4, outs):
        assert is_sentinel(o[..., 1]), n


# ---- 4. mask and gather against their host statement --------------------------------------------------------------------------------------
BEFORE = (0, 2, 3, 4)                  # the input field that teacher value v replaces


def host_mask(f5, t4, members, key0, thr_act, thr_inact):
    """numpy statement of mw_member_sample_mask on host arrays (nz, ncol, nens): (mask, active, finite), flat."""
    nz, ncol, nens = f5[0].shape
    plane, nelem = ncol * nens, nz * ncol * nens
    t = np.arange(nelem, dtype=np.int64)
    up = np.where(t + plane < nelem, t + plane, t)
    listed = np.isin(t % nens, members)
    f = [a.ravel() for a in f5]
    g = [a.ravel() for a in t4]
    with np.errstate(invalid="ignore", over="ignore"):
        act = np.zeros(nelem, dtype=bool)
        for v in range(4):
            act |= np.abs(g[v] - f[BEFORE[v]]) > 1.e-10
        fin = np.ones(nelem, dtype=bool)
        for a in f:
            fin &= np.isfinite(a.astype(np.float32))
        for v in BEFORE:
            fin &= np.isfinite(f[v][up].astype(np.float32))
        for a in g:
            fin &= np.isfinite(a.astype(np.float32))
    draw = u01(np.uint64(key0) + t.astype(np.uint64))
    return listed & fin & (draw < np.where(act, thr_act, thr_inact)), act, fin


def host_records(f5, t4, elems):
    nz, ncol, nens = f5[0].shape
    plane, nelem = ncol * nens, nz * ncol * nens
    up = np.where(elems + plane < nelem, elems + plane, elems)
    ins = np.zeros((elems.size, 5, 2), dtype=np.float32)
    with np.errstate(over="ignore"):
        for v in range(5):
            ins[:, v, 0] = f5[v].ravel()[elems].astype(np.float32)
        for slot, v in enumerate(BEFORE):
            ins[:, slot, 1] = f5[v].ravel()[up].astype(np.float32)
        outs = np.stack([a.ravel()[elems].astype(np.float32) for a in t4], axis=1)
    return ins, outs


def device_mask(f5, t4, members, key0, thr_act, thr_inact):
    import torch
    from miniweatherml_amd import capi, modules
    nz, ncol, nens = f5[0].shape
    mask = torch.full((nz * ncol * nens,), 7, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().mw_member_sample_mask(nz, ncol, nens, len(members), (C.c_int * len(members))(*members), modules._field_ptr_array(f5),
                                                modules._field_ptr_array(t4), key0, thr_act, thr_inact, C.c_void_p(mask.data_ptr()), None))
    torch.cuda.synchronize()
    return mask.cpu().numpy()


def device_records(f5, t4, elems):
    import torch
    from miniweatherml_amd import capi, modules
    nz, ncol, nens = f5[0].shape
    e = torch.from_numpy(elems).cuda()
    ins = torch.full((elems.size, 5, 2), 9.0, dtype=torch.float32, device="cuda")
    outs = torch.full((elems.size, 4), 9.0, dtype=torch.float32, device="cuda")
    capi.check(capi.lib().mw_member_gather_samples(nz, ncol, nens, modules._field_ptr_array(f5), modules._field_ptr_array(t4),
                                                   C.c_void_p(e.data_ptr()), elems.size, C.c_void_p(ins.data_ptr()), C.c_void_p(outs.data_ptr()), None))
    torch.cuda.synchronize()
    return ins.cpu().numpy(), outs.cpu().numpy()


@pytest.mark.parametrize("shape", [(2, 1, 15, 3), (22, 3, 11, 5), (13, 9, 9, 4)], ids=lambda s: "x".join(map(str, s)))
def test_mask_and_gather_equal_their_host_statement(mw, shape):
    import torch
    nz, ny, nx, nens = shape
    ncol = ny * nx
    state = make_state(shape, seed=31 + nz)
    rng = np.random.default_rng(nz)
    f5 = [state[n].reshape(nz, ncol, nens).copy() for n in IN5]
    t4 = [f5[v].copy() for v in BEFORE]
    moved = rng.random((nz, ncol, nens)) < 0.4                                 # the active class: one teacher value differs by 1e-3 >> 1e-10
    for v in range(4):
        t4[v][moved & (rng.integers(0, 4, size=moved.shape) == v)] += 1.0e-3
    members = [1, nens - 1] if nens > 2 else [1]
    members = sorted(set(members))
    f5[3][nz - 1, ncol // 2, members[0]] = np.nan                              # a top-level input: its own record and the one below it
    t4[1][0, 0, members[-1]] = 1.0e39                                          # finite as fp64, inf as fp32
    f5[2][0, ncol - 1, 0] = np.nan                                             # (a member that is not listed: no concern of the mask)
    df5 = [torch.from_numpy(a).cuda() for a in f5]
    dt4 = [torch.from_numpy(a).cuda() for a in t4]
    nelem = nz * ncol * nens
    for seed in (1, 987654321):
        key0 = (seed * nelem) % 2 ** 64
        want, act, fin = host_mask(f5, t4, members, key0, 0.3, 0.1)
        listed = np.isin(np.arange(nelem) % nens, members)
        assert (act & listed).any() and (~act & listed).any() and (~fin & listed).sum() >= 3
        got = device_mask(df5, dt4, members, key0, 0.3, 0.1)
        assert np.array_equal(got, want.astype(np.uint8))
        assert not got[~listed].any() and got.any()
        # the records of the taken elements, of the planted ones and of every listed element of the top level
        top = np.flatnonzero(listed & (np.arange(nelem) >= (nz - 1) * ncol * nens))
        elems = np.concatenate([np.flatnonzero(want), np.flatnonzero(~fin & listed), top]).astype(np.int64)
        ins, outs = device_records(df5, dt4, elems)
        wi, wo = host_records(f5, t4, elems)
        assert ins.tobytes() == wi.tobytes() and outs.tobytes() == wo.tobytes()
        assert np.array_equal(ins[-top.size:, :4, 1], ins[-top.size:, [0, 2, 3, 4], 0], equal_nan=True)      # the level above the top is the top


# ---- 5. the harvester ------------------------------------------------------------------------------------------------------------------
def harvester_on(state, directory, members, names, dt=DT, **kw):
    from miniweatherml_amd import modules
    c = make_coupler(*state["temp"].shape, modules.Microphysics_Kessler())
    load(c, state)
    h = modules.RolloutHarvester()
    os.makedirs(directory, exist_ok=True)
    h.init(c, names, members, str(directory), **kw)
    return h, c, h.harvest(c, dt, 0.0)


def test_harvester_files(mw, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    shape = (13, 9, 9, 4)
    nz, ncol, nens = shape[0], shape[1] * shape[2], shape[3]
    state = make_state(shape, seed=41)
    before = device(state)
    runs = [harvester_on(state, tmp_path / d, [1, 3], ["a", "b"], samples_per_step=200, seed=5) for d in ("one", "two")]
    h, c, added = runs[0]
    for n in IN5:
        assert same(fields(c, IN5)[n], before[n]), n
    assert added == runs[1][2] and h.skipped == {"a": 0, "b": 0}
    for name in ("a", "b"):
        assert open(h.files[name], "rb").read() == open(runs[1][0].files[name], "rb").read()
        assert os.path.basename(h.files[name]) == "rollout_samples_%s.nc" % name
    # the counts are the mask's: the host statement on the harvester's own teacher values, thresholds and key
    f5 = [state[n].reshape(nz, ncol, nens) for n in IN5]
    t4 = [t.cpu().numpy().reshape(nz, ncol, nens) for t in h._teacher]
    thr = h.thresholds(c)
    ncell = nz * ncol
    assert thr == (min(1.0, 0.5 * 200.0 / (0.4 * ncell)), min(1.0, (1 - 0.5) * 200.0 / ((1 - 0.4) * ncell)))      # DataGenerator's formulas
    want, _, _ = host_mask(f5, t4, [1, 3], (5 * nz * ncol * nens) % 2 ** 64, *thr)
    elems = np.flatnonzero(want)
    assert np.array_equal(h.last_elems, elems)
    for name, m in (("a", 1), ("b", 3)):
        assert added[name] == int((elems % nens == m).sum()) > 0
        for stencil in (False, True):
            ins, outs, meta = st.read_samples([h.files[name]], stencil=stencil)
            assert ins.shape == (added[name], 9 if stencil else 5) and outs.shape == (added[name], 4) and meta["time_step_size"] == DT
        wi, wo = host_records(f5, t4, elems[elems % nens == m])
        ins, outs, _ = st.read_samples([h.files[name]], stencil=True)
        assert np.array_equal(ins, np.concatenate([wi[:, :, 0], wi[:, :4, 1]], axis=1)) and np.array_equal(outs, wo)
    # a second call appends, with another draw
    more = h.harvest(c, DT, DT)
    assert st.read_samples([h.files["a"]])[0].shape[0] == added["a"] + more["a"] == h.samples["a"]
    assert not np.array_equal(h.last_elems, elems)


def test_harvester_skips_a_member_past_the_cap(mw, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    state = make_state((12, 3, 11, 3), seed=3, rain=False)
    state["precip_liquid"][..., 1] = 1.0e-2 * state["density_dry"][..., 1]
    h, c, added = harvester_on(state, tmp_path, [1, 2], ["wet", "dry"], dt=300.0, samples_per_step=200, seed=2, max_rainsplit=4)
    assert added["wet"] == 0 and h.skipped == {"wet": 1, "dry": 0} and added["dry"] > 0
    assert not (h.last_elems % 3 == 1).any()
    with pytest.raises(st.SurrogateTrainError, match="zero samples"):
        st.data_scaling(*st.read_samples([h.files["wet"]])[:2])


# ---- 6. the rollout step ------------------------------------------------------------------------------------------------------------------
def test_rollout_step_is_unchanged_by_harvesting(mw, tmp_path):
    from miniweatherml_amd import modules, surrogate_train as st
    shape = (13, 9, 9, 4)
    state = make_state(shape, seed=51)
    models = [nets(5)[0], nets(9)[0]]
    got = []
    for harvest in (False, True):
        micro = modules.Microphysics_Rollout()
        c = make_coupler(*shape, micro, models=models, persistence=True)
        load(c, state)
        assert micro.harvester is None and micro.harvest_now is False
        if harvest:
            micro.harvester = modules.RolloutHarvester()
            micro.harvester.init(c, micro.member_names[1:3], [1, 2], str(tmp_path), samples_per_step=100, seed=3)
            micro.harvest_now = True
        micro.time_step(c, DT)
        got.append(fields(c))
        if harvest:
            assert micro.harvester.calls == 1 and all(v > 0 for v in micro.harvester.samples.values())
            # the teacher saw the state the models were about to replace: the samples' inputs are the step's input state
            ins = st.read_samples(list(micro.harvester.files.values()))[0]
            assert np.isin(ins[:, 0], state["temp"][..., 1:3].astype(np.float32)).all()
    for n in ALL8 + ("precl",):
        assert same(got[0][n], got[1][n]), n


# ---- 7. the experiment ------------------------------------------------------------------------------------------------------------------
def test_driver_harvests_and_leaves_the_run_alone(mw, tmp_path, monkeypatch):
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from miniweatherml_amd import driver, surrogate_train as st
    entries, _ = write_models(tmp_path)
    entries = entries[:2]                                                       # one model of each width
    lst = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    monkeypatch.chdir(tmp_path)
    path, _ = write_yaml(tmp_path, nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=lst + "harvest: {interval: 2, samples_per_step: 200, seed: 1}\n")
    _, _, info = driver.run("rollout_surrogates", path, max_steps=4, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    hv = doc["harvest"]
    assert info["steps"] == 4 and hv["calls"] == 2 and hv["interval"] == 2 and hv["members"] == ["single_a", "stencil_a"]
    for name in ("single_a", "stencil_a"):
        assert hv["files"][name] == os.path.join(os.getcwd(), "rollout_samples_%s.nc" % name) and os.path.exists(hv["files"][name])
        n = st.read_samples([hv["files"][name]])[0].shape[0]
        assert n == hv["samples"][name] > 0 and hv["skipped"][name] == 0
    path, _ = write_yaml(tmp_path, nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=lst)
    driver.run("rollout_surrogates", path, max_steps=4, quiet=True)
    plain = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert "harvest" not in plain and plain["report"] == doc["report"] and plain["history"] == doc["history"]


# ---- 8. the warm start ------------------------------------------------------------------------------------------------------------------
def test_warm_start_continues_the_directory(mw, tmp_path):
    from test_gpu_surrogate_train import kessler_like
    from test_surrogate_train_cpu import write_sample_file
    from miniweatherml_amd import modules, surrogate_train as st
    ins, outs = kessler_like(6000, 2)
    f = write_sample_file(tmp_path / "s.nc", [(ins, outs)])
    d = str(tmp_path / "first")
    st.train_surrogate([f], d, epochs=3, batch_size=256, seed=4)
    ref = modules.load_surrogate_weights(*[os.path.join(d, x) for x in ("weights.txt", "input_scaling.txt", "output_scaling.txt")])
    w_file = np.concatenate([np.ravel(x) for x in ref[:4]])
    # more data than the directory's tables saw: the tables stay the directory's
    ins2, outs2 = kessler_like(6000, 3)
    ins2[:, 0] *= 1.05
    f2 = write_sample_file(tmp_path / "s2.nc", [(ins2, outs2)])
    warm = st.train_surrogate([f, f2], None, epochs=1, batch_size=256, seed=4, models=2, init=d)
    cold = st.train_surrogate([f, f2], None, epochs=1, batch_size=256, seed=4, models=2)
    assert warm["init"] == d and warm["initial_weights"].shape == (2, 104)
    assert np.array_equal(warm["initial_weights"][0], w_file) and np.array_equal(warm["initial_weights"][1], w_file)
    assert np.array_equal(warm["input_scaling"], ref[4]) and np.array_equal(warm["output_scaling"], ref[5])
    assert not np.array_equal(cold["input_scaling"], ref[4]) and "init" not in cold
    for m in range(2):
        print("model %d: first-epoch loss warm %.4e, cold %.4e" % (m, warm["history"][m]["loss"][0], cold["history"][m]["loss"][0]))
        assert warm["history"][m]["loss"][0] < cold["history"][m]["loss"][0]
    assert not np.array_equal(warm["weights"][0], warm["weights"][1])          # (the two differ by their epoch shuffles)
    with pytest.raises(st.SurrogateTrainError, match="parameters"):
        st.train_surrogate([f], None, epochs=1, batch_size=256, stencil=True, init=d)
