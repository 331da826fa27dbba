"""Surface rain of every rollout member from its column water budget on the GPU: mw_member_column_water and
mw_member_surface_rain against a host loop bit for bit, the closure of the budget against Kessler's own precl, the rollout step that the
option only reads, mw_member_rain_table against numpy, Microphysics_Kessler_Surrogate's budget, and the rollout_surrogates driver.

"Equal in bits" is equality of the int64 views of fp64 arrays.  The host loop adds the levels in ascending order into one accumulator that
starts from +0.0, each level as (water_vapor + cloud_liquid) + precip_liquid, and multiplies by dz once at the end."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_surrogate_rollout import ALL8, make_coupler, make_state, load, fields, model_list, nets

pytestmark = pytest.mark.gpu

WATER = ("water_vapor", "cloud_liquid", "precip_liquid")
DT = 1.0


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def host(t):
    return t.detach().cpu().numpy().copy()


def host_water(v, c, r, dz):
    """(nz, ...) host fields -> (...) column water, the kernels' association."""
    acc = np.zeros(v.shape[1:])
    for k in range(v.shape[0]):
        acc = acc + ((v[k] + c[k]) + r[k])
    return dz * acc


def water_of(coupler):
    f = fields(coupler, WATER)
    return [host(f[n]) for n in WATER]


def water_state(nz, ncol, nens, seed):
    """The three water fields (nz, 1, ncol, nens) drawn over the shipped input-scaling ranges."""
    si = nets(5)[0][4]
    rng = np.random.default_rng(seed)
    return {name: rng.uniform(si[2 + i, 0], si[2 + i, 1], (nz, 1, ncol, nens)) for i, name in enumerate(WATER)}


# ---- 1. mw_member_column_water ------------------------------------------------------------------------------------------------------
WATER_SHAPES = [(1, 1, 1), (2, 1, 3), (3, 65, 2), (9, 64, 4), (37, 1000, 3), (100, 257, 5), (5, 7, 64)]


@pytest.mark.parametrize("nz,ncol,nens", WATER_SHAPES)
def test_column_water_bit_for_bit(mw, nz, ncol, nens):
    """Every shape: one level, fewer levels than the kernel loads ahead, a remainder after its groups of four, one column, a block and one
    more, 64 members.  Then one NaN and one inf in single cells: each shows in its own (column, member) and nowhere else."""
    from miniweatherml_amd import modules
    c = make_coupler(nz, 1, ncol, nens, modules.Microphysics_Kessler())
    st = water_state(nz, ncol, nens, seed=nz + ncol + nens)
    load(c, st)
    want = host_water(*[st[n] for n in WATER], c.get_dz())
    got = modules.member_column_water(c)
    assert tuple(got.shape) == (1, ncol, nens) and same_bits(host(got), want)
    assert np.all(want > 0.0)
    # into a buffer of the caller's
    import torch
    out = torch.full((1, ncol, nens), -7.0, dtype=torch.float64, device="cuda")
    assert modules.member_column_water(c, out=out).data_ptr() == out.data_ptr() and same_bits(host(out), want)
    # non-finite cells
    rng = np.random.default_rng(5)
    cells = [(int(rng.integers(nz)), int(rng.integers(ncol)), int(rng.integers(nens))) for _ in range(2)]
    if cells[0][1:] == cells[1][1:]:
        cells[1] = (cells[1][0], (cells[1][1] + 1) % ncol, (cells[1][2] + 1) % nens)
    if cells[0][1:] == cells[1][1:]:
        cells = cells[:1]                                                       # (one column of one member: the NaN alone)
    st["cloud_liquid"][cells[0][0], 0, cells[0][1], cells[0][2]] = np.nan
    if len(cells) > 1:
        st["precip_liquid"][cells[1][0], 0, cells[1][1], cells[1][2]] = np.inf
    load(c, st)
    got = host(modules.member_column_water(c))[0]
    clean = np.ones((ncol, nens), dtype=bool)
    assert np.isnan(got[cells[0][1:]])
    clean[cells[0][1:]] = False
    if len(cells) > 1:
        assert got[cells[1][1:]] == np.inf
        clean[cells[1][1:]] = False
    assert np.array_equal(bits(got)[clean], bits(want[0])[clean])


# ---- 2. mw_member_surface_rain ------------------------------------------------------------------------------------------------------
FINISH_CASES = [((2, 1, 3), [1], [1], 0.5), ((3, 65, 2), [1], [0, 1], 60.0), ((9, 64, 4), [3, 1], [0, 1, 2, 3], 0.5),
                ((37, 1000, 3), [1, 2], [1, 2], 60.0), ((100, 257, 5), [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 0.5), ((5, 7, 64), [63, 5, 17], [0, 63, 5, 17, 40], 60.0),
                ((1, 1, 1), [0], [0], 60.0), ((9, 64, 4), [2], [], 0.5), ((9, 64, 4), [], [1, 3], 60.0)]


@pytest.mark.parametrize("shape,members,accum,dt", FINISH_CASES)
def test_finish_bit_for_bit(mw, shape, members, accum, dt):
    """Two calls on two states after two W_before: precl of the listed members is the host formula, every other member keeps its
    sentinel, rain_total grows by dt * (whatever precl holds) for the members of accum -- equal to the list, a superset, empty, alone."""
    import torch
    from miniweatherml_amd import modules
    nz, ncol, nens = shape
    c = make_coupler(nz, 1, ncol, nens, modules.Microphysics_Kessler())
    rng = np.random.default_rng(sum(shape))
    precl0 = rng.uniform(1.0, 2.0, (1, ncol, nens))
    total0 = rng.uniform(-1.0, 1.0, (1, ncol, nens))
    load(c, {"precl": precl0})
    total = torch.from_numpy(total0.copy()).cuda()
    want_p, want_t = precl0.copy(), total0.copy()
    for call in range(2):
        st = water_state(nz, ncol, nens, seed=100 * call + nz)
        load(c, st)
        after = host_water(*[st[n] for n in WATER], c.get_dz())
        before = after * rng.uniform(0.9, 1.2, after.shape)                      # (a member may have gained water: the sign is kept)
        for m in members:
            want_p[..., m] = (before[..., m] - after[..., m]) / (1000.0 * dt)
        for m in accum:
            want_t[..., m] = want_t[..., m] + dt * want_p[..., m]
        modules.member_surface_rain(c, members, accum, dt, torch.from_numpy(before).cuda(), total if accum else None)
        assert same_bits(host(fields(c, ("precl",))["precl"]), want_p), call
        assert same_bits(host(total), want_t), call
    if members:
        assert np.any(want_p[..., members] < 0.0) or ncol * len(members) < 4


def test_finish_and_column_water_entry_checks(mw):
    """Every refusal names its reason, launches nothing and leaves precl, rain_total and w as they were."""
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    nz, ncol, nens = 4, 16, 3
    f = [torch.rand((nz, ncol, nens), dtype=torch.float64, device="cuda") for _ in range(3)]
    wb = torch.rand((ncol, nens), dtype=torch.float64, device="cuda")
    precl = torch.full((ncol, nens), 3.0, dtype=torch.float64, device="cuda")
    total = torch.full((ncol, nens), 5.0, dtype=torch.float64, device="cuda")
    w = torch.full((ncol, nens), 7.0, dtype=torch.float64, device="cuda")
    ptrs = modules._field_ptr_array(f)
    holed = modules._field_ptr_array(f)
    holed[1] = None
    P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    ints = lambda *v: (C.c_int * max(1, len(v)))(*v)                            # noqa: E731

    def rain(nz=nz, ncol=ncol, nens=nens, members=(1,), accum=(0, 1, 2), water=ptrs, dz=500.0, dt=1.0, wb=P(wb), precl=P(precl), total=P(total),
             nm=None, na=None):
        return L.mw_member_surface_rain(nz, ncol, nens, len(members) if nm is None else nm, ints(*members), len(accum) if na is None else na,
                                        ints(*accum), water, dz, dt, wb, precl, total, None)

    def water(nz=nz, ncol=ncol, nens=nens, water=ptrs, dz=500.0, w=P(w)):
        return L.mw_member_column_water(nz, ncol, nens, water, dz, w, None)

    cases = [(lambda: rain(nz=0), "nz and ncol must be >= 1"), (lambda: rain(ncol=0), "nz and ncol must be >= 1"),
             (lambda: rain(nens=0), r"nens must be in \[1, 64\]"), (lambda: rain(nens=65), r"nens must be in \[1, 64\]"),
             (lambda: rain(members=(3,)), r"member 3 is outside \[0, 3\)"), (lambda: rain(members=(-1,)), r"member -1 is outside \[0, 3\)"),
             (lambda: rain(accum=(0, 4)), r"member 4 is outside \[0, 3\)"),
             (lambda: rain(members=(1, 1)), "member 1 is listed twice in members"), (lambda: rain(accum=(2, 0, 2)), "member 2 is listed twice in accum"),
             (lambda: rain(nm=4, members=(0, 1, 2, 2)), "members holds 4 members"), (lambda: rain(na=-1), "accum holds -1 members"),
             (lambda: rain(dt=0.0), "dt must be positive and finite"), (lambda: rain(dt=-1.0), "dt must be positive and finite"),
             (lambda: rain(dt=float("inf")), "dt must be positive and finite"), (lambda: rain(dt=float("nan")), "dt must be positive and finite"),
             (lambda: rain(dz=0.0), "dz must be positive and finite"), (lambda: rain(dz=float("nan")), "dz must be positive and finite"),
             (lambda: rain(dz=float("inf")), "dz must be positive and finite"),
             (lambda: rain(water=None), "null pointer"), (lambda: rain(water=holed), "null field"), (lambda: rain(wb=None), "null pointer"),
             (lambda: rain(precl=None), "null pointer"), (lambda: rain(total=None), "null pointer"),
             (lambda: water(nz=0), "nz and ncol must be >= 1"), (lambda: water(nens=65), r"nens must be in \[1, 64\]"),
             (lambda: water(dz=-500.0), "dz must be positive and finite"), (lambda: water(dz=float("inf")), "dz must be positive and finite"),
             (lambda: water(water=None), "null pointer"), (lambda: water(water=holed), "null field"), (lambda: water(w=None), "null pointer")]
    for call, msg in cases:
        with pytest.raises(modules.MWError, match=msg):
            capi.check(call())
    torch.cuda.synchronize()
    assert bool((precl == 3.0).all()) and bool((total == 5.0).all()) and bool((w == 7.0).all())
    # what is allowed: no rain_total without accum, no w_before without members, nothing at all
    assert rain(accum=(), total=None) == 0 and rain(members=(), wb=None) == 0 and rain(members=(), accum=(), wb=None, total=None) == 0
    torch.cuda.synchronize()
    assert bool((precl[:, 0] == 3.0).all()) and bool((precl[:, 2] == 3.0).all()) and not bool((precl[:, 1] == 3.0).any())
    # the wrappers refuse what the kernel cannot be given
    c = make_coupler(nz, 1, ncol, nens, modules.Microphysics_Kessler())
    with pytest.raises(modules.MWError, match="w_before must be"):
        modules.member_surface_rain(c, [1], [], 1.0, wb.view(-1))
    with pytest.raises(modules.MWError, match="out must be"):
        modules.member_column_water(c, out=w)


# ---- 3. closure against Kessler's own precl -------------------------------------------------------------------------------------------
CLOSURE_CASES = [(2, 500.0, 1.0, False), (9, 500.0, 1.0, False), (37, 500.0, 1.0, False), (37, 500.0, 60.0, True), (64, 150.0, 40.0, True)]
CLOSURE_COLUMNS = 40


def closure_state(nz, dz, nens, seed):
    """A physical state (nz, 1, CLOSURE_COLUMNS, nens) whose top level holds no rain."""
    rng = np.random.default_rng(seed)
    shape = (nz, 1, CLOSURE_COLUMNS, nens)
    z = ((np.arange(nz) + 0.5) * dz).reshape(nz, 1, 1, 1)
    H = nz * dz
    u = lambda a, b: rng.uniform(a, b, shape)                                   # noqa: E731
    st = {"temp": 300.0 - 0.0065 * z * (12000.0 / H) + u(-1.0, 1.0)}
    st["density_dry"] = 1.15 * np.exp(-1.5 * z / H) * u(0.98, 1.02)
    st["water_vapor"] = st["density_dry"] * 0.014 * np.exp(-5.0 * z / H) * u(0.5, 1.3)
    st["cloud_liquid"] = np.where(z < 0.7 * H, st["density_dry"] * u(0.0, 2.0e-3), 0.0)
    st["precip_liquid"] = st["density_dry"] * u(0.0, 5.0e-3)
    st["precip_liquid"][nz - 1] = 0.0
    for n in ("uvel", "vvel", "wvel"):
        st[n] = np.zeros(shape)
    st["precl"] = np.full(shape[1:], -1.0)
    return st


@pytest.mark.parametrize("nz,dz,dt,subcycled", CLOSURE_CASES)
def test_budget_closes_against_kesslers_own_precl(mw, nz, dz, dt, subcycled):
    """A two-member rollout, Kessler and persistence, with kessler among the budget members, against the same run without the option:
    per column |budget - Kessler's precl| <= (3 nz + 16) * 2^-52 * W_before / (1000 dt) -- 3 nz for the two sequential sums of nz terms
    and the sum inside Kessler, 16 for Kessler's roundings of the sedimentation term per cell; derived, not fitted.  Both Kessler forms
    (production and strict).  The largest multiple of 2^-52 * W_before / (1000 dt) seen is printed (DESIGN.md 13.8 records it)."""
    from miniweatherml_amd import modules
    st = closure_state(nz, dz, 2, seed=nz + int(dt))
    for strict in (0, 1):
        runs = []
        for option in (None, {"budget_members": ["kessler", "persistence"]}):
            micro = modules.Microphysics_Rollout()
            c = make_coupler(nz, 1, CLOSURE_COLUMNS, 2, micro, models=[], persistence=True)
            c.set_grid(100.0 * CLOSURE_COLUMNS, 100.0, dz * nz)
            assert c.get_dz() == dz
            load(c, st)
            micro.set_strict(strict)
            micro.surface_rain = option
            w_before = host(modules.member_column_water(c))
            micro.time_step(c, dt)
            runs.append((fields(c), micro))
        (off, _), (on, micro_on) = runs
        for n in ALL8:
            assert same_bits(host(on[n]), host(off[n])), n
        kessler, budget = host(off["precl"])[0, :, 0], host(on["precl"])[0, :, 0]
        unit = 2.0 ** -52 * w_before[0, :, 0] / (1000.0 * dt)
        worst = float(np.max(np.abs(budget - kessler) / unit))
        print("closure nz %d dz %g dt %g strict %d: largest |budget - precl| = %.3g units of eps W_before / (1000 dt), bound %d; "
              "max precl %.6e, max |budget - precl| / max precl %.3g"
              % (nz, dz, dt, strict, worst, 3 * nz + 16, kessler.max(), float(np.max(np.abs(budget - kessler)) / kessler.max())))
        assert np.any(kessler > 0.0) and np.all(np.isfinite(kessler)) and np.all(np.isfinite(budget))
        assert np.all(np.abs(budget - kessler) <= (3 * nz + 16) * unit), worst
        assert np.all(bits(host(on["precl"])[0, :, 1]) == 0)                      # persistence: +0.0
        assert same_bits(host(micro_on.rain_total), dt * host(on["precl"]))
        # the sub-cycled form is really reached where the case says so
        alone = modules.Microphysics_Kessler()
        ca = make_coupler(nz, 1, CLOSURE_COLUMNS, 1, alone)
        ca.set_grid(100.0 * CLOSURE_COLUMNS, 100.0, dz * nz)
        load(ca, st, 0)
        alone.set_strict(strict)
        rs = alone.time_step(ca, dt, return_rainsplit=True)
        assert (rs > 1) == subcycled, rs
        assert same_bits(host(fields(ca, ("precl",))["precl"])[0, :, 0], kessler)


# ---- 4. the rollout step is only read -------------------------------------------------------------------------------------------------
GUARD = {"temp": 0.05, "precip_liquid": 1.0e-5, "max_rainsplit": 64}
STEP_CASES = [((2, 1, 15, 3), "single", 1, True, None), ((2, 1, 15, 3), "stencil", 1, True, None), ((2, 1, 15, 3), "mixed", 2, False, None),
              ((22, 3, 11, 5), "mixed", 3, True, None), ((22, 3, 11, 5), "single", 4, False, None), ((22, 3, 11, 5), "single", 2, True, "mean"),
              ((22, 3, 11, 5), "stencil", 2, True, "guarded"), ((13, 9, 9, 4), "stencil", 2, False, "guarded"), ((13, 9, 9, 4), "single", 1, True, "mean"),
              ((13, 9, 9, 4), "mixed", 2, True, None)]


@pytest.mark.parametrize("shape,kind,k,persistence,committee", STEP_CASES,
                         ids=["%s-%s%d-%s-%s" % ("x".join(map(str, s)), kind, k, "pers" if p else "nopers", c) for s, kind, k, p, c in STEP_CASES])
def test_rollout_step_is_only_read(mw, shape, kind, k, persistence, committee):
    """Two steps with the option on beside two with it off: the eight fields and member 0's precl keep their bits; every budget member's
    precl is the host budget of the off run's fields before and after the step; persistence gets +0.0; rain_total is the host's sum."""
    from miniweatherml_amd import modules
    nz, ny, nx, nens = shape
    models = model_list(kind, k)
    names = ["m%d" % i for i in range(k)]
    committees = [] if committee is None else [("com", names) + ((GUARD,) if committee == "guarded" else ())]
    assert nens == 1 + k + len(committees) + int(persistence)
    state = make_state(shape, seed=sum(shape) + k)
    off, on = modules.Microphysics_Rollout(), modules.Microphysics_Rollout()
    c_off = make_coupler(nz, ny, nx, nens, off, models=models, persistence=persistence, names=names, committees=committees)
    c_on = make_coupler(nz, ny, nx, nens, on, models=models, persistence=persistence, names=names, committees=committees)
    load(c_off, state)
    load(c_on, state)
    on.surface_rain = {}
    assert off.surface_rain is None and off.rain_total is None
    total = np.zeros((ny, nx, nens))
    dz = c_off.get_dz()
    for step in range(2):
        before = host_water(*water_of(c_off), dz)
        off.time_step(c_off, DT)
        on.time_step(c_on, DT)
        after = host_water(*water_of(c_off), dz)
        f_off, f_on = fields(c_off), fields(c_on)
        for n in ALL8:
            assert same_bits(host(f_on[n]), host(f_off[n])), (n, step)
        p_off, p_on = host(f_off["precl"]), host(f_on["precl"])
        assert same_bits(p_on[..., 0], p_off[..., 0]), step
        want = (before - after) / (1000.0 * DT)
        assert np.all(np.isfinite(want))
        assert same_bits(p_on[..., 1:], want[..., 1:]), step
        if step == 0:                                                           # without the option the other members' precl is never written
            assert same_bits(p_off[..., 1:], state["precl"][..., 1:])
        if persistence:
            assert np.all(bits(p_on[..., nens - 1]) == 0), step
        assert np.any(p_on[..., 1] != 0.0)
        total = total + DT * p_on
        assert same_bits(host(on.rain_total), total), step
    assert off.rain_total is None
    with pytest.raises(modules.MWError, match="budget_members"):
        on.surface_rain = {"members": ["m0"]}
        on.time_step(c_on, DT)
    with pytest.raises(modules.MWError, match="distinct members"):
        on.surface_rain = {"budget_members": ["nobody"]}
        on.time_step(c_on, DT)


# ---- 5. mw_member_rain_table ------------------------------------------------------------------------------------------------------------
THRESHOLDS8 = [0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 25.0, 50.0]


def host_table(x, thr):
    """(ncol, nens) values, thresholds -> (len(thr), nens, 5) counts with numpy."""
    fin = np.isfinite(x) & np.isfinite(x[:, :1])
    out = np.zeros((len(thr), x.shape[1], 5), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j, q in enumerate(thr):
            fc, ob = x >= q, x[:, :1] >= q
            out[j, :, 0] = (fin & fc & ob).sum(0)
            out[j, :, 1] = (fin & ~fc & ob).sum(0)
            out[j, :, 2] = (fin & fc & ~ob).sum(0)
            out[j, :, 3] = (fin & ~fc & ~ob).sum(0)
            out[j, :, 4] = (~fin).sum(0)
    return out


def table_field(ncol, nens, thr, rng):
    """Values around the thresholds, a third of them EQUAL to one, with -0.0, NaN, +inf and -inf in members and a NaN in member 0."""
    x = rng.uniform(0.0, 2.0 * thr[-1], (ncol, nens)) * rng.choice([0.01, 0.1, 1.0], (ncol, nens))
    pick = rng.random((ncol, nens)) < 1.0 / 3.0
    x[pick] = rng.choice(thr, int(pick.sum()))
    e = nens - 1
    for i, v in enumerate((-0.0, np.nan, np.inf, -np.inf)):
        x[(3 + 5 * i) % ncol, (e + i) % nens if nens > 2 else e] = v
    x[(7 * ncol) // 8, 0] = np.nan                                               # takes the column out for every member
    if ncol > 2:
        x[1, 0] = thr[0]                                                        # an observation equal to a threshold is an event
        x[1, e] = np.nextafter(thr[0], 0.0)                                     # ... and one unit below it is none: a miss
    return x


@pytest.mark.parametrize("ncol", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("nens", [2, 3, 5, 64])
def test_rain_table_exactly(mw, ncol, nens):
    import torch
    from miniweatherml_amd import modules
    c = make_coupler(1, 1, 1, nens, modules.Microphysics_Kessler())
    rng = np.random.default_rng(1000 * nens + ncol)
    for nt in (1, 8):
        for nf in (1, 4):
            thr = [[q * (f + 1) for q in (THRESHOLDS8[2:3] if nt == 1 else THRESHOLDS8)] for f in range(nf)]
            xs = [table_field(ncol, nens, thr[f], rng) for f in range(nf)]
            got = modules.member_rain_table(c, [torch.from_numpy(x).cuda() for x in xs], thr)
            assert len(got) == nf
            for f in range(nf):
                assert got[f].dtype == np.int64 and got[f].shape == (nt, nens, 5)
                assert np.array_equal(got[f], host_table(xs[f], thr[f])), (nt, nf, f)
                assert np.all(got[f].sum(axis=2) == ncol)
                assert np.all(got[f][:, 0, 1:3] == 0)                           # member 0 never misses itself
    if ncol > 2:
        assert got[0][0, nens - 1, 1] >= 1 and np.all(got[0][:, :, 4] >= 1)


def test_rain_table_entry_checks(mw):
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    ncol, nens = 20, 3
    x = [torch.rand((ncol, nens), dtype=torch.float64, device="cuda") for _ in range(4)]
    ws = torch.zeros(L.mw_member_rain_table_workspace_bytes(ncol, nens, 4) // 8, dtype=torch.float64, device="cuda")
    counts = torch.full((4 * 8 * nens * 5,), -1, dtype=torch.int64, device="cuda")
    ptrs = modules._field_ptr_array(x)
    holed = modules._field_ptr_array(x)
    holed[0] = None
    P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731

    def table(ncol=ncol, nens=nens, nf=2, f=ptrs, nt=(2, 3), thr=(0.1, 0.2, 0, 0, 0, 0, 0, 0, 0.1, 0.5, 0.7), ws=P(ws), counts=P(counts), no_nt=False,
              no_thr=False):
        t = list(thr) + [0.0] * (32 - len(thr))
        return L.mw_member_rain_table(ncol, nens, nf, f, None if no_nt else (C.c_int * 4)(*(list(nt) + [0] * (4 - len(nt)))),
                                      None if no_thr else (C.c_double * 32)(*t), ws, counts, None)

    nan, inf = float("nan"), float("inf")
    for call, msg in ((lambda: table(ncol=0), "ncol must be >= 1"), (lambda: table(nens=0), r"nens must be in \[1, 64\]"),
                      (lambda: table(nens=65), r"nens must be in \[1, 64\]"), (lambda: table(nf=0), r"nf must be in \[1, 4\]"),
                      (lambda: table(nf=5), r"nf must be in \[1, 4\]"), (lambda: table(nt=(0, 3)), "field 0 has 0"),
                      (lambda: table(nt=(2, 9)), "field 1 has 9"), (lambda: table(thr=(0.1, nan)), "threshold 1 of field 0 is not finite"),
                      (lambda: table(thr=(inf, 0.2)), "threshold 0 of field 0 is not finite"),
                      (lambda: table(thr=(0.2, 0.2)), "field 0 are not strictly ascending"),
                      (lambda: table(thr=(0.1, 0.2, 0, 0, 0, 0, 0, 0, 0.1, 0.5, 0.4)), "field 1 are not strictly ascending"),
                      (lambda: table(f=None), "null pointer"), (lambda: table(f=holed), "null field"), (lambda: table(no_nt=True), "null pointer"),
                      (lambda: table(no_thr=True), "null pointer"), (lambda: table(ws=None), "null pointer"),
                      (lambda: table(counts=None), "null pointer")):
        with pytest.raises(modules.MWError, match=msg):
            capi.check(call())
    torch.cuda.synchronize()
    assert bool((counts == -1).all())
    for bad in ((0, 3, 1), (20, 0, 1), (20, 65, 1), (20, 3, 0), (20, 3, 5)):
        assert L.mw_member_rain_table_workspace_bytes(*bad) == 0
    assert table() == 0
    torch.cuda.synchronize()
    got = counts.cpu().numpy().reshape(4, 8, nens, 5)
    assert np.all(got[:2].sum(axis=3)[0, :2] == ncol) and np.all(got[1, :3].sum(axis=2) == ncol)
    assert np.all(got[0, 2:] == 0) and np.all(got[1, 3:] == 0) and np.all(got[2:] == -1)      # rows past nt: zeros; fields past nf: not written
    c = make_coupler(1, 1, 1, nens, modules.Microphysics_Kessler())
    with pytest.raises(modules.MWError, match="1 to 4 fields"):
        modules.member_rain_table(c, x[:2], [[0.1]])
    with pytest.raises(modules.MWError, match="1 to 4 fields"):
        modules.member_rain_table(c, x[:1], [[]])
    with pytest.raises(modules.MWError, match="members last"):
        modules.member_rain_table(c, [x[0], x[1][:10]], [[0.1], [0.1]])


# ---- 6. Microphysics_Kessler_Surrogate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 3, 11, 2), (22, 1, 15, 3)])
def test_online_surrogate_budget(mw, shape):
    """online with surface_rain: precl is the host budget of the state before the call and the state the network left, every member's
    columns alike; the state keeps the bits it has without the option.  online = False with the option is refused."""
    from miniweatherml_amd import modules
    nz, ny, nx, nens = shape
    state = make_state(shape, seed=sum(shape))
    out = []
    for option in (False, True):
        micro = modules.Microphysics_Kessler_Surrogate()
        c = make_coupler(nz, ny, nx, nens, micro)
        load(c, state)
        micro.online, micro.surface_rain = True, option
        for _ in range(2):
            before = host_water(*water_of(c), c.get_dz())
            micro.time_step(c, DT)
            after = host_water(*water_of(c), c.get_dz())
        out.append((fields(c), (before - after) / (1000.0 * DT)))
    (off, _), (on, want) = out
    for n in ALL8:
        assert same_bits(host(on[n]), host(off[n])), n
    assert same_bits(host(on["precl"]), want) and np.all(np.isfinite(want)) and np.any(want != 0.0)
    assert not same_bits(host(off["precl"]), want)                              # (without the option precl is Kessler's)
    micro = modules.Microphysics_Kessler_Surrogate()
    c = make_coupler(nz, ny, nx, nens, micro)
    load(c, state)
    micro.surface_rain = True
    with pytest.raises(modules.MWError, match="needs online = True"):
        micro.time_step(c, DT)


# ---- 7. the driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_surface_rain(mw, tmp_path, monkeypatch):
    """rollout_surrogates on the 16 x 12 x 10 grid of test_driver_rollout_surrogates with the block: the JSON's surface_rain has one entry
    per scoring step and member, the map is 1000 * rain_total as (nens, ny, nx); without the block: no key, no map, the same state."""
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from miniweatherml_amd import driver, modules
    entries, _ = write_models(tmp_path)
    extra = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries[:2])
    members = ["kessler", "single_a", "stencil_a", "persistence"]
    runs = {}
    for name, block in (("on", "surface_rain: {thresholds_mm_h: [0.1, 1, 5], thresholds_mm: [0.0001, 0.01], map: true}\n"), ("off", ""),
                        ("nomap", "surface_rain: {map: false}\n")):
        d = tmp_path / name
        d.mkdir()
        path, _ = write_yaml(d, nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra + block)
        monkeypatch.chdir(d)
        coupler, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
        runs[name] = (fields(coupler, ALL8), info, json.load(open(os.path.join(str(d), "surrogate_rollout.json"))), str(d))
    f_on, info, doc, d_on = runs["on"]
    rain = doc["surface_rain"]
    assert rain["thresholds_mm_h"] == [0.1, 1.0, 5.0] and rain["thresholds_mm"] == [0.0001, 0.01] and rain["map"] is True
    assert [t["step"] for t in rain["report"]] == [0, 1, 2] == [t["step"] for t in doc["report"]]
    for t in rain["report"]:
        assert list(t["members"]) == members == doc["members"]
        for m in members:
            assert list(t["members"][m]) == ["rate_mm_h", "accumulation_mm"]
            assert [q["threshold"] for q in t["members"][m]["rate_mm_h"]["thresholds"]] == [0.1, 1.0, 5.0]
            for q in t["members"][m]["accumulation_mm"]["thresholds"]:
                assert sum(q[k] for k in modules.RAIN_COUNTS) == 16 * 12
        assert t["members"]["persistence"]["rate_mm_h"]["max"] == 0.0 and t["members"]["persistence"]["rate_mm_h"]["min"] == 0.0
    got = np.load(os.path.join(d_on, "surrogate_rollout_rain.npy"))
    want = 1000.0 * host(info["rain_total"])
    assert got.dtype == np.float64 and got.shape == (4, 12, 16) and same_bits(got, np.ascontiguousarray(want.transpose(2, 0, 1)))
    last = rain["report"][-1]["members"]
    for k, m in enumerate(members):
        assert last[m]["accumulation_mm"]["mean"] == pytest.approx(float(got[k].mean()), rel=1e-12, abs=1e-300)
    f_off, info_off, doc_off, d_off = runs["off"]
    assert "surface_rain" not in doc_off and not os.path.exists(os.path.join(d_off, "surrogate_rollout_rain.npy")) and "rain_total" not in info_off
    assert {k: v for k, v in doc.items() if k not in ("surface_rain", "yaml")} == {k: v for k, v in doc_off.items() if k != "yaml"}
    for n in ALL8:
        assert same_bits(host(f_on[n]), host(f_off[n])), n
    _, _, doc_nomap, d_nomap = runs["nomap"]
    assert doc_nomap["surface_rain"]["map"] is False and doc_nomap["surface_rain"]["thresholds_mm"] == [0.1, 1.0, 5.0, 10.0, 25.0]
    assert not os.path.exists(os.path.join(d_nomap, "surrogate_rollout_rain.npy"))
