"""The surrogate rollout on the GPU: Microphysics_Rollout (Kessler, one network per member, persistence) against what exists, composed by
hand -- member slices made contiguous with torch, Microphysics_Kessler on a nens = 1 coupler, mlp_forward / mlp_stencil_forward per
model -- bit for bit; mw_member_divergence against exactly rounded host sums; the rollout_surrogates experiment.

"Equal" is torch.equal on the int64 views of the fp64 tensors throughout: the same bits, NaN included."""
import functools
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
OUT4 = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")
WINDS = ("uvel", "vvel", "wvel")
ALL8 = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor", "cloud_liquid", "precip_liquid")
SHAPES = [(1, 1, 1, 2), (2, 1, 15, 3), (9, 1, 1, 4), (22, 3, 11, 5), (13, 9, 9, 4), (37, 25, 40, 3)]
DT = 1.0


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# ---- models and states ----------------------------------------------------------------------------------------------------------------
_NETS = {}


def nets(n_in):
    """Six models of one width with two pairs of scaling tables (test_gpu_surrogate_eval.model_pool)."""
    from test_gpu_surrogate_eval import model_pool
    if n_in not in _NETS:
        _NETS[n_in] = model_pool(n_in, 6)
    return _NETS[n_in]


def model_list(kind, k):
    """k models: all single-cell, all stencil, or alternating (stencil first, so that neither bank's members are contiguous)."""
    if kind == "single":
        return [nets(5)[i] for i in range(k)]
    if kind == "stencil":
        return [nets(9)[i] for i in range(k)]
    return [nets(9 if i % 2 == 0 else 5)[i // 2] for i in range(k)]


def make_coupler(nz, ny, nx, nens, micro, **init):
    """A coupler with the dycore's five fields and the microphysics' tracers, without a dycore (which needs nz, nx >= 3)."""
    from miniweatherml_amd.coupler import Coupler
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(nz, ny, nx, nens)
    c.set_grid(100.0 * nx, 100.0 * ny, 500.0 * nz)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry",) + WINDS + ("temp",):
        dm.register_and_allocate(name, name, (nz, ny, nx, nens), ["z", "y", "x", "nens"])
    micro.init(c, **init)
    return c


def make_state(shape, seed, rain=True):
    """Host fields (nz, ny, nx, nens) drawn over the shipped scaling ranges, every member different, and a precl full of sentinels."""
    si = nets(5)[0][4]
    rng = np.random.default_rng(seed)
    st = {name: rng.uniform(si[i, 0], si[i, 1], shape) for i, name in enumerate(IN5)}
    if not rain:
        st["precip_liquid"][...] = 0.0
    for name in WINDS:
        st[name] = rng.uniform(-10.0, 10.0, shape)
    st["precl"] = rng.uniform(1.0, 2.0, shape[1:])
    return st


def load(coupler, state, member=None):
    """Writes a host state (or one member of it, into a nens = 1 coupler) to the coupler's fields."""
    import torch
    dm = coupler.get_data_manager_readwrite()
    for name, a in state.items():
        a = a if member is None else a[..., member:member + 1]
        dm.get(name).copy_(torch.from_numpy(np.ascontiguousarray(a)))


def members_of(state, idx):
    """The state with the members `idx`, in that order."""
    return {n: np.ascontiguousarray(v[..., idx]) for n, v in state.items()}


def fields(coupler, names=ALL8 + ("precl",)):
    dm = coupler.get_data_manager_readonly()
    return {n: dm.get(n, True).clone() for n in names}


def kessler_alone(state, member, strict, dt=DT, return_rainsplit=False):
    """Microphysics_Kessler on a nens = 1 coupler that holds one member of the state: (fields, rainsplit); an MWError is returned, not
    raised (Kessler needs two levels)."""
    from miniweatherml_amd import modules
    nz, ny, nx, _ = state["temp"].shape
    micro = modules.Microphysics_Kessler()
    c = make_coupler(nz, ny, nx, 1, micro)
    load(c, state, member)
    micro.set_strict(strict)
    try:
        rs = micro.time_step(c, dt, return_rainsplit=return_rainsplit)
    except modules.MWError as e:
        return e, None
    return fields(c), rs


def forward_alone(state, member, net, strict):
    """The existing forward kernels on one member's contiguous slices: the four outputs (nz, ny, nx)."""
    import torch
    from miniweatherml_amd import modules
    nz = state["temp"].shape[0]
    ins = [torch.from_numpy(np.ascontiguousarray(state[n][..., member])).cuda() for n in IN5]
    if net[0].shape[0] == 9:
        outs = modules.mlp_stencil_forward(nz, *[t.view(nz, -1) for t in ins], *net, strict=strict)
    else:
        outs = modules.mlp_forward(*ins, *net, strict=strict)
    return [o.view(ins[0].shape) for o in outs]


def rollout_step(state, models, persistence, strict, dt=DT):
    """One Microphysics_Rollout.time_step on the state: (fields after, the MWError of the Kessler member or None).  Where Kessler refuses
    the grid (nz = 1) the models are still applied, through the module's own banks."""
    from miniweatherml_amd import modules
    nz, ny, nx, nens = state["temp"].shape
    micro = modules.Microphysics_Rollout()
    c = make_coupler(nz, ny, nx, nens, micro, models=models, persistence=persistence)
    load(c, state)
    micro.set_strict(strict)
    micro.mlp_strict = strict
    err = None
    try:
        micro.time_step(c, dt)
    except modules.MWError as e:
        err = e
        dm = c.get_data_manager_readwrite()
        for bank, members in micro.banks:
            bank.strict = strict
            bank.members_apply(nz, members, [dm.get(n) for n in IN5])
    return fields(c), err


def check_step(state, models, persistence, strict):
    import torch
    nens = state["temp"].shape[-1]
    got, err = rollout_step(state, models, persistence, strict)
    before = {n: torch.from_numpy(np.ascontiguousarray(a)).cuda() for n, a in state.items()}
    # member 0 and its precl: the nens = 1 Kessler result (or the same refusal)
    want, _ = kessler_alone(state, 0, strict)
    if isinstance(want, Exception):
        assert err is not None and "nz >= 2" in str(err) and "nz >= 2" in str(want)
        for n in ALL8 + ("precl",):
            assert same(got[n][..., 0], before[n][..., 0]), n
    else:
        assert err is None
        for n in ALL8 + ("precl",):
            assert same(got[n][..., 0], want[n][..., 0]), (n, "kessler member")
    # members 1 .. K: the forward kernels' outputs
    for k, net in enumerate(models):
        outs = forward_alone(state, 1 + k, net, strict)
        for n, o in zip(OUT4, outs):
            assert same(got[n][..., 1 + k], o), (n, "model member", 1 + k, net[0].shape[0])
    # untouched: the persistence member, density_dry, the winds, precl beyond member 0
    if persistence:
        for n in ALL8:
            assert same(got[n][..., nens - 1], before[n][..., nens - 1]), (n, "persistence member")
    for n in ("density_dry",) + WINDS:
        assert same(got[n], before[n]), n
    assert same(got["precl"][..., 1:], before["precl"][..., 1:])


def step_cases():
    out = []
    for shape in SHAPES:
        for persistence in (True, False):
            k = shape[3] - 1 - int(persistence)
            for kind in (["none"] if k == 0 else ["single", "stencil"] + (["mixed"] if k >= 2 else [])):
                out.append(pytest.param(shape, persistence, kind, id="%s-%s-%s" % ("x".join(map(str, shape)), "pers" if persistence else "nopers", kind)))
    return out


@pytest.mark.parametrize("shape,persistence,kind", step_cases())
def test_step_equals_the_composed_form(mw, shape, persistence, kind):
    """Every shape with and without the persistence member, banks of one width and mixed, both strict settings (mlp_strict and the Kessler
    strict flag together).  nz = 1 and 2, nz no z chunk of the forward divides, cell counts off every multiple of 16 / 32 / 64, odd member
    counts.  With nz = 1 Kessler refuses the grid in both forms (it needs two levels): member 0 must then be untouched, and the models
    are applied through the module's banks."""
    k = shape[3] - 1 - int(persistence)
    models = model_list(kind, k)
    state = make_state(shape, seed=sum(shape) + 7 * k)
    for strict in (0, 1):
        check_step(state, models, persistence, strict)


def test_kessler_member_is_isolated_from_the_others(mw):
    """Member 1 carries so much rain that Kessler over ALL members sub-cycles (rainsplit > 1, taken from the minimum over the columns of the
    call); member 0 has none.  The rollout's member 0 still equals the nens = 1 result, which has rainsplit 1."""
    from miniweatherml_amd import modules
    shape = (12, 3, 11, 3)
    state = make_state(shape, seed=3, rain=False)
    state["precip_liquid"][..., 1] = 1.0e-2 * state["density_dry"][..., 1]
    dt = 300.0                                                         # dz = 500 m: the rain of member 1 falls faster than 0.8 dz / dt = 1.3 m/s
    micro = modules.Microphysics_Kessler()
    c = make_coupler(*shape, micro)
    load(c, state)
    assert micro.time_step(c, dt, return_rainsplit=True) > 1
    want, rs = kessler_alone(state, 0, 0, dt, return_rainsplit=True)
    assert rs == 1
    got, err = rollout_step(state, [nets(5)[0]], True, 0, dt)
    assert err is None
    together = fields(c)
    for n in OUT4 + ("precl",):
        assert same(got[n][..., 0], want[n][..., 0]), n
    assert not same(together["temp"][..., 0], want["temp"][..., 0])    # (the premise: stepped with the others, member 0 differs)


def test_model_order_and_copies(mw):
    """(A, B) against (B, A) with the two members' inputs swapped: member 1 of one run is member 2 of the other.  Two copies of one model on
    two members with the same input: identical members."""
    shape = (13, 9, 9, 4)
    a, b = nets(5)[1], nets(9)[2]
    state = make_state(shape, seed=11)
    swapped = members_of(state, [0, 2, 1, 3])
    ab, _ = rollout_step(state, [a, b], True, 0)
    ba, _ = rollout_step(swapped, [b, a], True, 0)
    for n in OUT4:
        assert same(ab[n][..., 1], ba[n][..., 2]) and same(ab[n][..., 2], ba[n][..., 1]), n
    twin = members_of(state, [0, 1, 1, 3])
    for net in (a, b):
        got, _ = rollout_step(twin, [net, net], True, 0)
        for n in OUT4:
            assert same(got[n][..., 1], got[n][..., 2]), n


def test_a_member_does_not_depend_on_its_neighbours(mw):
    """Model B between A and C of a mixed list, and alone in a rollout of its own: the same member."""
    shape = (22, 3, 11, 5)
    state = make_state(shape, seed=12)
    for b in (nets(5)[2], nets(9)[1]):
        full, _ = rollout_step(state, [nets(9)[0], b, nets(5)[0]], True, 0)
        alone, _ = rollout_step(members_of(state, [0, 2, 4]), [b], True, 0)
        for n in OUT4:
            assert same(full[n][..., 2], alone[n][..., 1]), n


@pytest.mark.parametrize("n_in", [5, 9])
def test_nan_weights_stay_in_their_member(mw, n_in):
    """A model whose layer-2 weights are NaN: its own member is what the forward kernel makes of such a model (temp NaN everywhere; the
    water outputs pass fmax(0, NaN) = 0), every other member keeps the bits of the run with the healthy model, and member_divergence counts
    that member's non-finite elements exactly and shows NaN in its sums and extrema.  Step level only: no dycore sees the NaN."""
    import torch
    from miniweatherml_amd import modules
    shape = (9, 3, 11, 4)
    n = 9 * 3 * 11
    well = nets(n_in)[1]
    sick = well[:2] + (np.full_like(well[2], np.nan),) + well[3:]
    others = [nets(5)[0], nets(9)[0]]
    state = make_state(shape, seed=13)
    ref, _ = rollout_step(state, [others[0], well, others[1]], False, 0)
    for strict in (0, 1):
        got, _ = rollout_step(state, [others[0], sick, others[1]], False, strict)
        assert torch.isnan(got["temp"][..., 2]).all()
        for name, o in zip(OUT4, forward_alone(state, 2, sick, strict)):
            assert same(got[name][..., 2], o), name
        if strict == 0:
            for name in ALL8 + ("precl",):
                assert same(got[name][..., [0, 1, 3]], ref[name][..., [0, 1, 3]]), name
    # the divergence of the stepped state
    micro = modules.Microphysics_Rollout()
    c = make_coupler(*shape, micro, models=[others[0], sick, others[1]], persistence=False)
    load(c, state)
    micro.time_step(c, DT)
    stats, nonf = modules.member_divergence(c, ALL8)
    it = ALL8.index("temp")
    want = np.zeros((4, 8), dtype=np.int64)
    want[2, it] = n
    assert np.array_equal(nonf, want)
    assert np.isnan(stats[2, it]).all()
    assert np.isfinite(np.delete(stats.reshape(32, 7), 2 * 8 + it, axis=0)).all()
    rep = modules.rollout_report(stats, nonf, n, micro.member_names, ALL8)
    assert rep["model1"]["finite"] is False and rep["model1"]["fields"]["temp"]["nonfinite"] == n and rep["model0"]["finite"] is True
    json.dumps(rep, allow_nan=False)


def test_entry_point_errors(mw):
    import ctypes as C
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    bank = modules.SurrogateBank([nets(5)[0], nets(5)[1]])
    f = [torch.zeros((4, 16, 3), dtype=torch.float64, device="cuda") for _ in range(5)]
    ptrs = modules._field_ptr_array(f)
    for members, msg in (((1, 3), b"outside [0, 3)"), ((-1, 1), b"outside [0, 3)"), ((2, 2), b"given to two models")):
        assert L.mw_surrogate_members_apply(bank._h, (C.c_int * 2)(*members), 4, 16, 3, ptrs, None) != 0 and msg in L.mw_last_error()
    assert L.mw_surrogate_members_apply(bank._h, (C.c_int * 2)(1, 2), 0, 16, 3, ptrs, None) != 0 and b"must be >= 1" in L.mw_last_error()
    ptrs[3] = None
    assert L.mw_surrogate_members_apply(bank._h, (C.c_int * 2)(1, 2), 4, 16, 3, ptrs, None) != 0 and b"null field" in L.mw_last_error()
    with pytest.raises(modules.MWError, match="2 models"):
        bank.members_apply(4, [1], f)
    micro = modules.Microphysics_Rollout()
    with pytest.raises(modules.MWError, match="need nens = 4, the coupler has 3"):
        make_coupler(4, 1, 16, 3, micro, models=[nets(5)[0], nets(9)[0]], persistence=True)


# ---- mw_member_divergence ---------------------------------------------------------------------------------------------------------------
def divergence_cases():
    out = []
    for nens in (2, 3, 5):
        for n in (1, 63, 64, 65, 257, 1025, 512 * (256 // nens) + 1):      # the last: one cell past the grid-stride threshold
            for nf in (1, 8):
                out.append((n, nens, nf))
    return out


def host_divergence(vals):
    """(stats (nens, nf, 7), bound (nens, nf, 7)) from host fields (nf, n, nens): exactly rounded sums, bound = n * 2^-52 * sum |terms|
    for the four sums (of d and of |d| that is the exact sum of |d|) and 0 for the extrema."""
    nf, n, nens = vals.shape
    stats, bound = np.zeros((nens, nf, 7)), np.zeros((nens, nf, 7))
    for m in range(nens):
        for f in range(nf):
            x = vals[f, :, m]
            d = x - vals[f, :, 0]
            sa, s2, sax = math.fsum(np.abs(d)), math.fsum(d * d), math.fsum(np.abs(x))
            stats[m, f] = [math.fsum(d), sa, s2, np.max(np.abs(d)), math.fsum(x), np.min(x), np.max(x)]
            bound[m, f, [0, 1, 2, 4]] = n * 2.0 ** -52 * np.array([sa, sa, s2, sax])
    return stats, bound


@pytest.mark.parametrize("n,nens,nf", divergence_cases())
def test_divergence_against_exact_host_sums(mw, n, nens, nf):
    """Sums within n * 2^-52 * sum |terms| of math.fsum (the bound of a fixed-order fp64 sum of n terms, DESIGN.md section 13:
    k_surrogate_sums), extrema and counts exact, two calls the same bytes, member 0's d statistics exactly 0."""
    from miniweatherml_amd import modules
    rng = np.random.default_rng(1000 * nens + n + nf)
    vals = rng.normal(size=(8, n, nens)) * 10.0 ** rng.uniform(-3, 3, size=(8, n, nens))
    c = make_coupler(1, 1, n, nens, modules.Microphysics_Kessler())
    load(c, {name: vals[f].reshape(1, 1, n, nens) for f, name in enumerate(ALL8)})
    names = ALL8[:nf] if nf == 8 else (ALL8[5],)
    sel = vals if nf == 8 else vals[5:6]
    stats, nonf = modules.member_divergence(c, names)
    again, nonf2 = modules.member_divergence(c, names)
    assert stats.tobytes() == again.tobytes() and nonf.tobytes() == nonf2.tobytes()
    assert stats.shape == (nens, nf, 7) and nonf.shape == (nens, nf) and nonf.dtype == np.int64 and not nonf.any()
    want, bound = host_divergence(sel)
    err = np.abs(stats - want)
    print("n %d nens %d nf %d: worst |sum - fsum| / bound = %.3g" % (n, nens, nf, np.max(err / np.where(bound > 0, bound, 1.0))))
    assert np.all(err <= bound), (err, bound)
    assert np.array_equal(stats[..., [3, 5, 6]], want[..., [3, 5, 6]])
    assert np.all(stats[0, :, :4] == 0.0)


def test_divergence_counts_and_propagates_non_finite_values(mw):
    """NaN and inf elements are counted per member and field; NaN reaches the sums and all three extrema (fmax would drop it), an inf the
    maximum; an inf of member 0 makes its own d there NaN (inf - inf) and every other member's infinite."""
    from miniweatherml_amd import modules
    n, nens = 300, 3
    rng = np.random.default_rng(5)
    vals = rng.normal(size=(8, n, nens))
    vals[4, 17, 1] = np.nan
    vals[4, 290, 1] = np.nan
    vals[5, 100, 2] = np.inf
    vals[6, 7, 0] = -np.inf
    c = make_coupler(1, 1, n, nens, modules.Microphysics_Kessler())
    load(c, {name: vals[f].reshape(1, 1, n, nens) for f, name in enumerate(ALL8)})
    stats, nonf = modules.member_divergence(c, ALL8)
    want = np.zeros((nens, 8), dtype=np.int64)
    want[1, 4], want[2, 5], want[0, 6] = 2, 1, 1
    assert np.array_equal(nonf, want)
    assert np.isnan(stats[1, 4]).all() and np.isfinite(stats[[0, 2], 4]).all()
    assert stats[2, 5, 6] == np.inf and stats[2, 5, 3] == np.inf and stats[2, 5, 0] == np.inf and np.isfinite(stats[2, 5, 5])
    assert stats[0, 6, 5] == -np.inf and np.isnan(stats[0, 6, :4]).all() and np.all(stats[1, 6, :4] == np.inf) and np.isfinite(stats[1, 6, 4:]).all()
    assert np.isfinite(stats[:, [0, 1, 2, 3, 7]]).all()


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def test_driver_rollout_surrogates(mw, tmp_path, monkeypatch):
    """driver.run("rollout_surrogates") on the 16 x 12 x 10 grid of test_driver_evaluate_surrogates with three models of both widths, two of
    them the same network: the JSON's last history entry is member_divergence of the returned coupler, the two twins end bitwise
    identical, and the persistence member's water has left the Kessler member's."""
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from miniweatherml_amd import driver, modules
    entries, _ = write_models(tmp_path)
    entries = [entries[0], entries[1], dict(entries[0], name="single_a_twin")]
    extra = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    path, _ = write_yaml(tmp_path, nens=5, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
    monkeypatch.chdir(tmp_path)
    coupler, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert info["steps"] == 3 and [h["step"] for h in doc["history"]] == [0, 1, 2] and coupler.get_nens() == 5
    assert doc["members"] == ["kessler", "single_a", "stencil_a", "single_a_twin", "persistence"] and doc["fields"] == list(ALL8)
    assert [m["member"] for m in doc["models"]] == [1, 2, 3] and set(doc["diverged_at"]) == set(doc["members"])
    assert len(doc["report"]) == 3 and doc["report"][-1]["step"] == 2
    stats, nonf = modules.member_divergence(coupler, ALL8)
    assert np.array_equal(np.array(doc["history"][-1]["stats"]), stats) and doc["history"][-1]["nonfinite"] == nonf.tolist()
    now = fields(coupler, ALL8)
    for n in ALL8:
        assert same(now[n][..., 1], now[n][..., 3]), n
    water = [float((now[n][..., 4] - now[n][..., 0]).abs().max()) for n in ("water_vapor", "cloud_liquid", "precip_liquid")]
    print("max |persistence - kessler| of the three water fields:", water)
    assert max(water) > 0.0
    monkeypatch.setattr(driver, "_distributed", lambda device: (2, 0, device))
    with pytest.raises(ValueError, match="one rank"):
        driver.run("rollout_surrogates", path, max_steps=1, quiet=True)


def test_kessler_member_equals_an_all_kessler_ensemble(mw):
    """Member 0 of a rollout against member 0 of a run of the same nens in which Kessler steps every member (Kessler strict, three steps of
    the supercell loop): no module couples the members -- the dycore, the sponge and the nudger keep one column per member, the time step
    depends on the grid alone -- so the two are the same bits."""
    from miniweatherml_amd import modules
    models = [nets(5)[0], nets(9)[0], nets(5)[1]]
    micro = modules.Microphysics_Rollout()
    micro.init = functools.partial(micro.init, models=models, persistence=True)
    runs = [modules.make_supercell(16, 12, 10, 5, 8000., 6000., 20000., micro=micro, with_nudger=True),
            modules.make_supercell(16, 12, 10, 5, 8000., 6000., 20000., with_nudger=True)]
    for coupler, dycore, mic, nudger in runs:
        mic.set_strict(1)
        for _ in range(3):
            modules.supercell_step(coupler, dycore, mic, nudger)
    a, b = fields(runs[0][0]), fields(runs[1][0])
    for n in ALL8 + ("precl",):
        scale = float(b[n][..., 0].abs().max())
        print("%s: max |rollout - all-Kessler| of member 0 = %.3g (max |field| %.3g)" % (n, float((a[n][..., 0] - b[n][..., 0]).abs().max()), scale))
    for n in ALL8 + ("precl",):
        assert same(a[n][..., 0], b[n][..., 0]), n
