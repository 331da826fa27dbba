"""The latent-heat closure on the GPU: mw_member_heat_closure against the numpy statement of its rule and of the order of
its sums (heat_closure_ref.py) bit for bit, the tolerance edge, the order-free sums, the call without the heating plane and with an empty
closed list, the entry checks; Kessler's own residual, strict and production; the rollout step, the online surrogate and the
rollout_surrogates driver.

"Equal in bits" is equality of the int64 views of fp64 arrays.  Every buffer the call writes -- temp, the workspace
(mw_member_heat_closure_workspace_bytes, exactly), counts, stats and the heating plane -- and every array it reads has TAIL sentinel
doubles behind it that must come back untouched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import heat_closure_ref as ref
from test_gpu_surface_rain import STEP_CASES, GUARD, WATER, bits, host, same_bits
from test_gpu_surrogate_rollout import ALL8, fields, load, make_coupler, make_state, model_list
from test_gpu_water_fix import SENTINEL, Guarded, ints, water_maker

pytestmark = pytest.mark.gpu

DZ = 137.5
READ = ("rho_d", "rho_v", "temp_before", "rho_v_before")


def call_closure(ta, rd, rva, tb, rvb, members, closed, tol, dz, dt, lv=ref.LV, cp_d=ref.CP_D, with_heating=True):
    """mw_member_heat_closure on guarded copies of host arrays: a dict of what every buffer holds afterwards."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    nz, ncol, nens = ta.shape
    b = {"temp": Guarded(ta), "rho_d": Guarded(rd), "rho_v": Guarded(rva), "temp_before": Guarded(tb), "rho_v_before": Guarded(rvb),
         "counts": Guarded(np.full((nens, 2), -5, dtype=np.int64)), "stats": Guarded(np.full((nens, 6), SENTINEL)),
         "heating": Guarded(np.full((ncol, nens), SENTINEL))}
    nbytes = L.mw_member_heat_closure_workspace_bytes(ncol, nens)
    assert nbytes == ((ncol * nens + 255) // 256) * nens * 64
    ws = Guarded(np.full(nbytes // 8, SENTINEL))
    before2 = (C.c_void_p * 2)(b["temp_before"].ptr.value, b["rho_v_before"].ptr.value)
    capi.check(L.mw_member_heat_closure(nz, ncol, nens, len(members), ints(members), len(closed), ints(closed), float(tol), float(lv), float(cp_d),
                                        float(dz), float(dt), b["temp"].ptr, b["rho_d"].ptr, b["rho_v"].ptr, before2, ws.ptr, b["counts"].ptr,
                                        b["stats"].ptr, b["heating"].ptr if with_heating else None, None))
    torch.cuda.synchronize()
    for g in list(b.values()) + [ws]:
        assert g.tail_clean()
    out = {k: g.host() for k, g in b.items()}
    for k, a in zip(READ, (rd, rva, tb, rvb)):
        assert same_bits(out[k], a), k
    return out


def lists_for(nens):
    """(members, closed, unlisted): the last member and member 0 closed, one member diagnosed but not closed, the rest in no list."""
    closed = [nens - 1] + ([0] if nens > 2 else [])
    extra = [e for e in range(nens) if e not in closed][:1]
    return closed + extra, closed, [e for e in range(nens) if e not in closed + extra]


def recipe(nz, ncol, nens, seed):
    """(ta, rd, rva, tb, rvb, planted): physical fields before, after = before + noise; the members in no list hold NaN in both
    before-fields; and, where the plane has room, on closed members: a NaN in temp_after, an inf in rho_v_after, rho_d == 0, a NaN in
    temp_before, and after == before for a whole column."""
    rng = np.random.default_rng(seed)
    _, closed, unlisted = lists_for(nens)
    shape = (nz, ncol, nens)
    tb, rd, rvb = rng.uniform(200.0, 310.0, shape), rng.uniform(0.05, 1.2, shape), rng.uniform(0.0, 2.0e-2, shape)
    ta, rva = tb + rng.normal(0.0, 0.5, shape), np.abs(rvb + rng.normal(0.0, 2.0e-4, shape))
    tb[..., unlisted] = np.nan
    rvb[..., unlisted] = np.nan
    planted = {}
    pairs = [(c, e) for c in range(ncol) for e in closed][::-1]
    if len(pairs) >= 10:
        planted.update(zip(("nan_after", "inf_vapour", "zero_density", "nan_before", "still"), pairs))
        ta[nz // 2][planted["nan_after"]] = np.nan
        rva[nz - 1][planted["inf_vapour"]] = np.inf
        rd[0][planted["zero_density"]] = 0.0
        tb[nz // 3][planted["nan_before"]] = np.nan
        c, e = planted["still"]
        ta[:, c, e], rva[:, c, e] = tb[:, c, e], rvb[:, c, e]
    return ta, rd, rva, tb, rvb, planted


# the last shape: 65,538 plane elements are 257 blocks, the smallest plane at which a thread of the final kernel (thread 0: block rows 0
# and 256) folds two rows; five levels are one look-ahead group and a tail.  Block 256 holds members 1 and 2 of the last column.
STRIDE = (5, 21846, 3)
SHAPES = [(1, 1, 1), (2, 1, 3), (3, 65, 2), (4, 64, 4), (5, 7, 64), (8, 255, 1), (9, 64, 4), (9, 257, 1), (37, 257, 3), STRIDE]
_CASES = {}


def case(shape):
    """The recipe, the call's result and the reference's for a shape, computed once and never changed."""
    if shape not in _CASES:
        nz, ncol, nens = shape
        arrays = recipe(nz, ncol, nens, seed=sum(shape))
        members, closed, _ = lists_for(nens)
        dt = 0.5 if nz % 2 else 60.0
        got = call_closure(*arrays[:5], members, closed, 0.0, DZ, dt)
        want = ref.closure(*arrays[:5], DZ, dt, members, closed, 0.0)
        _CASES[shape] = (arrays[:5], arrays[5], got, want, (members, closed), dt)
    return _CASES[shape]


# ---- 1. the kernel against the rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bit_for_bit(mw, shape):
    """nz below, at and above the look-ahead of four; planes below, at and above a wavefront and a block; bit 63 of the member mask.  Lanes
    of one plane element per thread put every member into every full wavefront, so the wavefronts without a listed lane are the last
    block's beyond the plane (1 x 1, 2 x 3, 65 x 2, 257 x 1, 257 x 3) and the one with a single listed lane is 257 x 1's fifth (and every
    wavefront of test_one_member_of_sixty_four).  temp, both counts, max |r|, max |H| and the heating plane are the reference's bits; the
    four sums are the bits of the reference's lanes folded in the kernels' order, and within n 2^-52 sum |x| of numpy's own order."""
    nz, ncol, nens = shape
    (ta, rd, rva, tb, rvb), planted, got, want, (members, closed), dt = case(shape)
    assert same_bits(got["temp"], want["temp"])
    assert np.array_equal(got["counts"], want["counts"])
    assert same_bits(got["heating"], want["heating"])
    assert same_bits(got["stats"][:, 3], want["max_r"]) and same_bits(got["stats"][:, 5], want["max_h"])
    assert same_bits(got["stats"], ref.kernel_order_stats(want["lanes"]))
    if shape == STRIDE:                                                         # row 256 is not a row of zeros: the loop's second turn adds something
        assert np.all(want["lanes"][-1, 1:, 1:4] > 0.0)
    r = np.where(np.isfinite(want["r"]), want["r"], 0.0)
    listed = np.zeros(nens, dtype=bool)
    listed[members] = True
    cells, eps = nz * ncol, 2.0 ** -52
    assert np.all(np.abs(got["stats"][:, 0] - want["stats"][:, 0]) <= cells * eps * np.abs(r).sum(axis=(0, 1)))
    assert np.all(np.abs(got["stats"][:, 1] - want["stats"][:, 1]) <= cells * eps * np.abs(r).sum(axis=(0, 1)))
    assert np.all(np.abs(got["stats"][:, 2] - want["stats"][:, 2]) <= cells * eps * (r * r).sum(axis=(0, 1)))
    assert np.all(np.abs(got["stats"][:, 4] - want["stats"][:, 4]) <= ncol * eps * np.abs(want["heating"]).sum(axis=0))
    # who was closed: every finite cell of a closed member that moved, no cell of any other member
    hit = want["closed_cells"]
    others = [e for e in range(nens) if e not in closed]
    assert hit[..., closed].any() and not hit[..., others].any()
    assert same_bits(got["temp"][..., others], ta[..., others])
    # a member diagnosed but not closed has statistics and no closed cell; a member in no list has nothing at all, NaN before-fields or not
    for e in members:
        if e not in closed:
            assert got["counts"][e, 0] == 0 and got["stats"][e, 3] > 0.0 and np.any(got["heating"][:, e] != 0.0)
    idle = [e for e in range(nens) if e not in members]
    assert np.all(got["counts"][idle] == 0) and np.all(bits(got["stats"][idle]) == 0) and np.all(bits(got["heating"][:, idle]) == 0)
    if planted:
        for name in ("nan_after", "inf_vapour", "zero_density", "nan_before"):
            c, e = planted[name]
            assert want["skipped_cells"][:, c, e].sum() == 1, name
        assert int(want["counts"][:, 1].sum()) == 4
        c, e = planted["nan_after"]
        assert np.isnan(got["temp"][nz // 2, c, e])                              # a NaN temp stays one
        c, e = planted["still"]
        assert np.all(bits(want["r"][:, c, e]) == 0) and bits(got["heating"][c, e]) == 0 and same_bits(got["temp"][:, c, e], ta[:, c, e])
        assert np.all(np.isfinite(got["stats"])) and np.all(np.isfinite(got["heating"]))


def test_one_member_of_sixty_four(mw):
    """nens = 64 with member 63 alone: every wavefront has a single listed lane, its last one (bit 63 of both masks)."""
    (ta, rd, rva, tb, rvb), _, _, _, _, dt = case((5, 7, 64))
    tb, rvb = tb.copy(), rvb.copy()
    tb[..., :63] = np.nan
    rvb[..., :63] = np.nan
    got = call_closure(ta, rd, rva, tb, rvb, [63], [63], 0.0, DZ, dt)
    want = ref.closure(ta, rd, rva, tb, rvb, DZ, dt, [63], [63], 0.0)
    assert same_bits(got["temp"], want["temp"]) and np.array_equal(got["counts"], want["counts"]) and same_bits(got["heating"], want["heating"])
    assert same_bits(got["stats"], ref.kernel_order_stats(want["lanes"])) and got["counts"][63, 0] > 0
    assert same_bits(got["temp"][..., :63], ta[..., :63]) and np.all(bits(got["stats"][:63]) == 0)


def test_without_the_heating_plane(mw):
    shape = (9, 64, 4)
    arrays, _, got, _, (members, closed), dt = case(shape)
    bare = call_closure(*arrays, members, closed, 0.0, DZ, dt, with_heating=False)
    for k in ("temp", "counts", "stats"):
        assert same_bits(bare[k].view(np.float64), got[k].view(np.float64)), k
    assert np.all(bare["heating"] == SENTINEL)


@pytest.mark.parametrize("shape", [(3, 65, 2), (9, 257, 1), (5, 7, 64)])
def test_empty_closed_list_writes_no_temp(mw, shape):
    """Diagnose only: no byte of temp is written, no cell is counted as closed, and the statistics -- of the residual before closing -- are
    those of the call that closes."""
    arrays, _, got, _, (members, _), dt = case(shape)
    bare = call_closure(*arrays, members, [], 0.0, DZ, dt)
    assert same_bits(bare["temp"], arrays[0]) and np.all(bare["counts"][:, 0] == 0)
    assert np.array_equal(bare["counts"][:, 1], got["counts"][:, 1])
    assert same_bits(bare["stats"], got["stats"]) and same_bits(bare["heating"], got["heating"])


def test_tolerance_edge(mw):
    """temp_before 1, no vapour change, temp 1.5: |r| = 0.5 == tolerance is not closed; with the next fp64 below 0.5 as the tolerance it is."""
    one = lambda x: np.full((1, 1, 1), x)                                       # noqa: E731
    args = (one(1.5), one(1.0), one(0.0), one(1.0), one(0.0), [0], [0])
    kept = call_closure(*args, 0.5, 1.0, 1.0)
    assert kept["counts"].tolist() == [[0, 0]] and kept["temp"][0, 0, 0] == 1.5
    assert kept["stats"][0].tolist() == [0.5, 0.5, 0.25, 0.5, 1003.0 * 0.5, 1003.0 * 0.5] and kept["heating"][0, 0] == 501.5
    edge = call_closure(*args, float(np.nextafter(0.5, 0.0)), 1.0, 1.0)
    assert edge["counts"].tolist() == [[1, 0]] and edge["temp"][0, 0, 0] == 1.0 and same_bits(edge["stats"], kept["stats"])


def test_sums_where_every_order_agrees(mw):
    """Fields on a 2^-10 grid, rho_d, C = lv / cp_d = 4, dz, dt and cp_d powers of two: every residual, every product and every partial sum
    is exact, so any order of the levels, lanes and blocks gives the same bits as numpy's."""
    nz, ncol, nens = 6, 700, 3
    rng = np.random.default_rng(11)
    shape = (nz, ncol, nens)
    tb, rvb = rng.integers(0, 65536, shape) / 1024.0, rng.integers(0, 64, shape) / 1024.0
    ta, rva = tb + rng.integers(-512, 513, shape) / 1024.0, rng.integers(0, 64, shape) / 1024.0
    rd = 2.0 ** rng.integers(-1, 2, shape)
    members, closed = [2, 0, 1], [1]
    got = call_closure(ta, rd, rva, tb, rvb, members, closed, 0.25, 128.0, 0.5, lv=4096.0, cp_d=1024.0)
    want = ref.closure(ta, rd, rva, tb, rvb, 128.0, 0.5, members, closed, 0.25, lv=4096.0, cp_d=1024.0)
    assert 100 < want["counts"][1, 0] < nz * ncol - 100 and np.all(want["counts"][[0, 2]] == 0)
    assert same_bits(got["temp"], want["temp"]) and np.array_equal(got["counts"], want["counts"]) and same_bits(got["heating"], want["heating"])
    assert same_bits(got["stats"], want["stats"])
    r = want["r"]
    exact = np.stack([r[::-1].sum(axis=(1, 0)), np.abs(r)[::-1].sum(axis=(1, 0)), (r * r)[::-1].sum(axis=(1, 0)), np.abs(r).max(axis=(0, 1)),
                      want["heating"][::-1].sum(axis=0), np.abs(want["heating"]).max(axis=0)], axis=1)
    assert same_bits(want["stats"], exact)                                      # (exact indeed)


# ---- 2. the entry checks -----------------------------------------------------------------------------------------------------------------
def test_entry_checks(mw):
    """Every refusal names its reason, launches nothing and leaves every buffer as it was."""
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    nz, ncol, nens = 4, 16, 3
    f = [torch.rand((nz, ncol, nens), dtype=torch.float64, device="cuda") + 0.5 for _ in range(5)]      # temp, rho_d, rho_v, temp_b, rho_v_b
    f0 = [t.clone() for t in f]
    full = lambda v, n: torch.full((n,), v, dtype=torch.float64, device="cuda")                          # noqa: E731
    heating, stats = full(11.0, ncol * nens), full(13.0, 6 * nens)
    counts = torch.full((2 * nens,), -1, dtype=torch.int64, device="cuda")
    ws = full(17.0, L.mw_member_heat_closure_workspace_bytes(ncol, nens) // 8)
    P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    pair = lambda a, b: (C.c_void_p * 2)(a, b)                                  # noqa: E731
    b2 = pair(f[3].data_ptr(), f[4].data_ptr())

    def go(nz=nz, ncol=ncol, nens=nens, members=(0, 1), closed=(1,), tol=0.0, lv=2.5e6, cp_d=1003.0, dz=500.0, dt=1.0, temp=P(f[0]), rho_d=P(f[1]),
           rho_v=P(f[2]), before2=b2, ws=P(ws), counts=P(counts), stats=P(stats), heating=P(heating), nclosed=None, nm=None):
        return L.mw_member_heat_closure(nz, ncol, nens, len(members) if nm is None else nm, ints(members), len(closed) if nclosed is None else nclosed,
                                        ints(closed), tol, lv, cp_d, dz, dt, temp, rho_d, rho_v, before2, ws, counts, stats, heating, None)

    nan, inf = float("nan"), float("inf")
    cases = [(lambda: go(nz=0), "nz and ncol must be >= 1"), (lambda: go(ncol=0), "nz and ncol must be >= 1"),
             (lambda: go(nens=0), r"nens must be in \[1, 64\]"), (lambda: go(nens=65), r"nens must be in \[1, 64\]"),
             (lambda: go(members=(3,)), r"member 3 is outside \[0, 3\)"), (lambda: go(closed=(-1,)), r"member -1 is outside \[0, 3\)"),
             (lambda: go(members=(1, 1)), "member 1 is listed twice in members"),
             (lambda: go(members=(0, 1, 2), closed=(1, 2, 1)), "member 1 is listed twice in closed"),
             (lambda: go(nclosed=4, closed=(0, 1, 2, 2)), "closed holds 4 members"), (lambda: go(nclosed=-1), "closed holds -1 members"),
             (lambda: go(nm=4, members=(0, 1, 2, 2)), "members holds 4 members"),
             (lambda: go(closed=(2,)), "member 2 is in closed but not in members"),
             (lambda: go(members=(), closed=(2,)), "member 2 is in closed but not in members"),
             (lambda: go(tol=-1.0e-300), "tolerance must be finite and >= 0"), (lambda: go(tol=nan), "tolerance must be finite and >= 0"),
             (lambda: go(tol=inf), "tolerance must be finite and >= 0"),
             (lambda: go(lv=0.0), "lv and cp_d must be positive and finite"), (lambda: go(lv=nan), "lv and cp_d must be positive and finite"),
             (lambda: go(cp_d=-1003.0), "lv and cp_d must be positive and finite"), (lambda: go(cp_d=inf), "lv and cp_d must be positive and finite"),
             (lambda: go(dt=0.0), "dt must be positive and finite"), (lambda: go(dt=inf), "dt must be positive and finite"),
             (lambda: go(dt=nan), "dt must be positive and finite"), (lambda: go(dz=0.0), "dz must be positive and finite"),
             (lambda: go(dz=-1.0), "dz must be positive and finite"), (lambda: go(dz=nan), "dz must be positive and finite"),
             (lambda: go(dz=inf), "dz must be positive and finite"),
             (lambda: go(temp=None), "null pointer"), (lambda: go(rho_d=None), "null pointer"), (lambda: go(rho_v=None), "null pointer"),
             (lambda: go(before2=None), "null pointer"), (lambda: go(before2=pair(f[3].data_ptr(), None)), "null field"),
             (lambda: go(ws=None), "null pointer"), (lambda: go(counts=None), "null pointer"), (lambda: go(stats=None), "null pointer"),
             (lambda: go(rho_d=P(f[0])), "only read"), (lambda: go(rho_v=P(f[0])), "only read"),
             (lambda: go(before2=pair(f[0].data_ptr(), f[4].data_ptr())), "only read"),
             (lambda: go(before2=pair(f[3].data_ptr(), f[0].data_ptr())), "only read")]
    for call, msg in cases:
        with pytest.raises(modules.MWError, match=msg):
            capi.check(call())
    torch.cuda.synchronize()
    assert all(bool((t == v).all()) for t, v in ((heating, 11.0), (stats, 13.0), (ws, 17.0), (counts, -1)))
    assert all(torch.equal(a, b) for a, b in zip(f, f0))
    for bad in ((0, 3), (16, 0), (16, 65)):
        assert L.mw_member_heat_closure_workspace_bytes(*bad) == 0
    # what is allowed: no heating plane, nothing closed, nothing listed at all (the statistics are still set)
    assert go(heating=None) == 0 and go(closed=()) == 0
    assert go(members=(), closed=()) == 0
    torch.cuda.synchronize()
    assert bool((counts == 0).all()) and bool((stats == 0.0).all()) and bool((heating == 0.0).all())
    assert all(torch.equal(a, b) for a, b in zip(f[1:], f0[1:]))
    # the wrappers refuse what the kernel cannot be given
    c = make_coupler(nz, 1, ncol, nens, modules.Microphysics_Kessler())
    with pytest.raises(modules.MWError, match="before2 must be"):
        modules.member_heat_closure(c, [1], [1], 1.0, [f[3], f[4]])


# ---- 3. Kessler obeys it -----------------------------------------------------------------------------------------------------------------
def kessler_on_gpu(nz, ncol, dz, dt, strict):
    """mw_kessler_time_step on ref.moist_state (the CPU test's states): (before, after, rainsplit, the new call's counts and stats)."""
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    st = ref.moist_state(nz, ncol, dz, seed=nz + int(dz))
    dev = {k: torch.from_numpy(a.copy()).cuda() for k, a in st.items()}
    before2 = [dev["temp"].clone(), dev["rho_v"].clone()]
    precl = torch.zeros(ncol, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(1, L.mw_kessler_workspace_bytes(nz, ncol) // 8 + 1), dtype=torch.float64, device="cuda")
    rs = C.c_int(0)
    P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    try:
        capi.check(L.mw_kessler_set_strict(strict))
        capi.check(L.mw_kessler_time_step(nz, ncol, dz, dt, P(dev["rho_v"]), P(dev["rho_c"]), P(dev["rho_r"]), P(dev["rho_d"]), P(dev["temp"]), P(precl),
                                          P(ws), C.byref(rs), None))
    finally:
        capi.check(L.mw_kessler_set_strict(0))
    out = modules.heat_closure_finish(dev["temp"], dev["rho_d"], dev["rho_v"], before2, nz, ncol, 1, [0], [], 0.0, dz, dt)
    stats, counts = out.host()
    return st, {k: host(t) for k, t in dev.items()}, rs.value, counts, stats


@pytest.mark.parametrize("strict,factor", [(1, 1), (0, 2)], ids=["strict", "production"])
@pytest.mark.parametrize("nz,ncol,dz,dt", ref.KESSLER_CASES)
def test_kessler_obeys_the_identity(mw, nz, ncol, dz, dt, strict, factor):
    """Strict Kessler is the oracle bit for bit, so the CPU bound (rainsplit + 4) ulp(temp) per cell holds as it stands; production
    contracts and reorders: twice that, one extra rounding per fused operation.  The kernel's max |r| is the host's."""
    before, after, rs, counts, stats = kessler_on_gpu(nz, ncol, dz, dt, strict)
    if dt > 1.0:
        assert rs > 1
    _, r = ref.residual(after["temp"], after["rho_d"], after["rho_v"], before["temp"], before["rho_v"])
    in_ulp = np.abs(r) / ref.ulp(after["temp"])
    print("%s kessler %dx%d dz %g dt %g: rainsplit %d, max |dT| %.3g K, max |r| %.3g K = %.3g ulp of temp (bound %d)"
          % ("strict" if strict else "production", nz, ncol, dz, dt, rs, np.abs(after["temp"] - before["temp"]).max(), np.abs(r).max(), in_ulp.max(),
             factor * (rs + 4)))
    assert counts.tolist() == [0, 0] and stats[3] == np.abs(r).max()
    assert np.abs(after["temp"] - before["temp"]).max() > 0.5
    assert np.all(np.abs(r) <= factor * ref.kessler_bound(rs, after["temp"]))


# ---- 4. the rollout step -----------------------------------------------------------------------------------------------------------------
def flat3(a, nens):
    return a.reshape(a.shape[0], -1, nens)


def run_step(shape, state, models, names, persistence, committees, closure=None, fixer=None):
    from miniweatherml_amd import modules
    nz, ny, nx, nens = shape
    micro = modules.Microphysics_Rollout()
    c = make_coupler(nz, ny, nx, nens, micro, models=models, persistence=persistence, names=names, committees=committees)
    load(c, state)
    micro.heat_closure, micro.water_fixer = closure, fixer
    micro.time_step(c, 1.0)
    return fields(c), micro, c


@pytest.mark.parametrize("shape,kind,k,persistence,committee", STEP_CASES,
                         ids=["%s-%s%d-%s-%s" % ("x".join(map(str, s)), kind, k, "pers" if p else "nopers", c) for s, kind, k, p, c in STEP_CASES])
def test_rollout_step(mw, shape, kind, k, persistence, committee):
    """One step from a dry state (model 0 is a constant model that makes water in every column) without the option, with it, with the
    water fixer, and with both.  Without it the new code is not reached; diagnosing alone writes nothing; a closed member's temp is the
    reference applied to (the state before, the state the step leaves without the option); the water fields and every other member keep
    the bits of the run without the key; with the fixer too, temp is the closure-only run's and the water fields are the fixer-only run's."""
    from miniweatherml_amd import modules
    nz, ny, nx, nens = shape
    models = model_list(kind, k)
    models[0] = water_maker(int(models[0][0].shape[0]), 0.05)
    names = ["m%d" % i for i in range(k)]
    committees = [] if committee is None else [("com", names) + ((GUARD,) if committee == "guarded" else ())]
    listed = ["m0"] + (["com"] if committee else [])
    wet = make_state(shape, seed=sum(shape) + k)
    state = {n: (0.01 * a if n in WATER else a) for n, a in wet.items()}
    args = (shape, state, models, names, persistence, committees)
    off, m_off, c_off = run_step(*args)
    assert m_off._heat_before is None and m_off._heat is None and m_off.heat_closure_reports() is None
    diag, m_diag, _ = run_step(*args, closure={"closed": []})
    on, m_on, _ = run_step(*args, closure={"closed": listed})
    fix, _, _ = run_step(*args, fixer={"members": listed})
    both, _, _ = run_step(*args, closure={"closed": listed}, fixer={"members": listed})
    for n in ALL8 + ("precl",):
        assert same_bits(host(diag[n]), host(off[n])), n
    diagnosed = [e for e in range(nens) if m_on.member_names[e] != "persistence"]
    closed = [m_on.member_names.index(n) for n in listed]
    want = ref.closure(flat3(host(off["temp"]), nens), flat3(host(off["density_dry"]), nens), flat3(host(off["water_vapor"]), nens),
                       flat3(state["temp"], nens), flat3(state["water_vapor"], nens), c_off.get_dz(), 1.0, diagnosed, closed, 0.0)
    for n in ALL8 + ("precl",):
        if n != "temp":
            assert same_bits(host(on[n]), host(off[n])), n
    assert same_bits(flat3(host(on["temp"]), nens), want["temp"])
    rest = [e for e in range(nens) if e not in closed]
    assert same_bits(host(on["temp"])[..., rest], host(off["temp"])[..., rest])
    assert want["closed_cells"][..., closed[0]].any()
    # with the fixer too: the closure saw the vapour the network made, the fixer the water
    assert same_bits(host(both["temp"]), host(on["temp"]))
    for n in WATER + ("precl",):
        assert same_bits(host(both[n]), host(fix[n])), n
    assert not same_bits(host(fix["water_vapor"]), host(off["water_vapor"]))
    # the records: of the residual before closing, the same with and without closing
    for micro, cl in ((m_on, closed), (m_diag, [])):
        micro.heat_closure_record(7)
        rep = micro.heat_closure_reports()
        assert rep["members"] == [micro.member_names[e] for e in diagnosed] and rep["closed"] == [micro.member_names[e] for e in cl]
        assert rep["cells"] == nz * ny * nx and rep["columns"] == ny * nx and [s["step"] for s in rep["steps"]] == [7]
        for e in diagnosed:
            row = rep["steps"][0]["members"][micro.member_names[e]]
            assert row["cells_closed"] == (int(want["counts"][e, 0]) if e in cl else 0) and row["cells_skipped"] == 0
            assert row["residual_K"]["max"] == float(want["max_r"][e]) and row["heating_W_m2"]["max"] == float(want["max_h"][e])
    if persistence:
        assert "persistence" not in rep["members"]
    for bad, msg in (({"member": ["m0"]}, "keys are members, closed and tolerance"), ({"closed": ["kessler"]}, "never kessler or persistence"),
                     ({"closed": ["m0", "m0"]}, "distinct network-stepped"), ({"members": ["kessler"], "closed": ["m0"]}, "must be among its members"),
                     ({"members": []}, "one or more distinct members"), ({"tolerance": -1.0}, "finite number >= 0")):
        m_on.heat_closure = bad
        with pytest.raises(modules.MWError, match=msg):
            m_on.heat_closure_reports()


def physical_state(shape, seed):
    """make_state's winds and precl around ref.moist_state's columns (dz = 500 m, make_coupler's): a state Kessler is at home on."""
    nz, ny, nx, nens = shape
    st = make_state(shape, seed)
    moist = ref.moist_state(nz, ny * nx * nens, 500.0, seed)
    for n, key in (("temp", "temp"), ("density_dry", "rho_d"), ("water_vapor", "rho_v"), ("cloud_liquid", "rho_c"), ("precip_liquid", "rho_r")):
        st[n] = np.ascontiguousarray(moist[key].reshape(shape))
    return st


def test_guarded_committee_with_every_column_flagged(mw):
    """Thresholds 0: Kessler takes every column of the guarded member, so its residual is Kessler's -- within the production bound, twice
    (rainsplit + 4) ulp(temp) -- and a tolerance of 1e-9 K leaves every bit of its temp alone, where tolerance 0 moves cells by ulps."""
    shape = (13, 9, 9, 4)
    nz, ny, nx, nens = shape
    models, names = model_list("single", 2), ["m0", "m1"]
    guard = dict(GUARD, temp=0.0, water_vapor=0.0, cloud_liquid=0.0, precip_liquid=0.0)
    args = (shape, physical_state(shape, 3), models, names, False, [("com", names, guard)])
    diag, m_diag, c = run_step(*args, closure={"members": ["com"], "closed": []})
    m_diag.guard_record(0, 1.0)
    step = m_diag.guard_reports()[0]["steps"][0]
    assert step["flagged"] == ny * nx and step["rainsplit"] >= 1
    e = m_diag.member_names.index("com")
    state = args[1]
    _, r = ref.residual(host(diag["temp"])[..., e], host(diag["density_dry"])[..., e], host(diag["water_vapor"])[..., e], state["temp"][..., e],
                        state["water_vapor"][..., e])
    temp = host(diag["temp"])[..., e]
    print("guarded member, every column Kessler's: rainsplit %d, max |dT| %.3g K, max |r| %.3g ulp of temp (bound %d)"
          % (step["rainsplit"], np.abs(temp - state["temp"][..., e]).max(), (np.abs(r) / ref.ulp(temp)).max(), 2 * (step["rainsplit"] + 4)))
    assert np.abs(temp - state["temp"][..., e]).max() > 0.5
    assert np.all(np.abs(r) <= 2 * ref.kessler_bound(step["rainsplit"], temp))
    m_diag.heat_closure_record(0)
    assert m_diag.heat_closure_reports()["steps"][0]["members"]["com"]["residual_K"]["max"] == np.abs(r).max()
    calm, m_calm, _ = run_step(*args, closure={"members": ["com"], "closed": ["com"], "tolerance": 1.0e-9})
    assert same_bits(host(calm["temp"]), host(diag["temp"]))
    m_calm.heat_closure_record(0)
    assert m_calm.heat_closure_reports()["steps"][0]["members"]["com"]["cells_closed"] == 0
    sharp, _, _ = run_step(*args, closure={"members": ["com"], "closed": ["com"]})
    moved = np.abs(host(sharp["temp"]) - host(diag["temp"]))[..., e]
    assert np.all(moved <= 2 * ref.kessler_bound(step["rainsplit"], temp))
    others = [m for m in range(nens) if m != e]
    assert same_bits(host(sharp["temp"])[..., others], host(diag["temp"])[..., others])


def test_twins_one_closed(mw):
    """Two members share one set of weights and one of them is closed: it reports a residual and closed cells, its twin keeps the bits of
    the run without the key, and a second, diagnose-only call on the state left behind finds max |r| == 0 for it."""
    import torch
    from miniweatherml_amd import modules
    shape = (9, 3, 11, 4)
    nz, ny, nx, nens = shape
    net = model_list("single", 2)[1]
    state = make_state(shape, seed=21)
    for n in ALL8 + ("precl",):                                                 # the twins start from one state too
        state[n][..., 2] = state[n][..., 1]
    args = (shape, state, [net, net], ["free", "closed"], True, [])
    off, _, _ = run_step(*args)
    on, micro, c = run_step(*args, closure={"closed": ["closed"]})
    micro.heat_closure_record(0)
    row = micro.heat_closure_reports()["steps"][0]["members"]
    assert row["closed"]["residual_K"]["max"] > 0.0 and row["closed"]["cells_closed"] > 0
    assert row["free"]["cells_closed"] == 0 and row["free"]["residual_K"] == row["closed"]["residual_K"]
    assert row["free"]["heating_W_m2"] == row["closed"]["heating_W_m2"]
    assert same_bits(host(on["temp"])[..., 1], host(off["temp"])[..., 1]) and same_bits(host(off["temp"])[..., 2], host(off["temp"])[..., 1])
    assert not same_bits(host(on["temp"])[..., 2], host(off["temp"])[..., 2])
    before2 = [torch.from_numpy(state[n]).cuda() for n in ("temp", "water_vapor")]
    heating = torch.full((ny, nx, nens), SENTINEL, dtype=torch.float64, device="cuda")
    counts, stats = modules.member_heat_closure(c, [2], [], 1.0, before2, heating=heating)
    assert counts.tolist() == [[0, 0]] * nens and np.all(bits(stats) == 0) and np.all(bits(host(heating)) == 0)
    counts, stats = modules.member_heat_closure(c, [1, 2], [], 1.0, before2)
    assert stats[1, 3] == row["free"]["residual_K"]["max"] and stats[2, 3] == 0.0


# ---- 5. the online surrogate -------------------------------------------------------------------------------------------------------------
def test_online_surrogate_heat_closure(mw):
    """online with heat_closure (a committee of one constant model): temp is the reference applied to the state before the call and what
    the network leaves without the option, the plane as one member; with the water fixer too the water fields are the fixer-only run's;
    online = False with the option is refused."""
    from miniweatherml_amd import modules
    shape = (9, 3, 11, 2)
    nz, ny, nx, nens = shape
    state = make_state(shape, seed=sum(shape))
    for n in WATER:
        state[n] = 0.6 * state[n]
    maker = [water_maker(5, 0.3)]
    out = {}
    for key, closure, fixer in (("off", None, None), ("on", True, None), ("fix", None, True), ("both", {"tolerance": 0.0}, True)):
        micro = modules.Microphysics_Kessler_Surrogate()
        c = make_coupler(nz, ny, nx, nens, micro, committee=maker)
        load(c, state)
        micro.online, micro.surface_rain, micro.heat_closure, micro.water_fixer = True, True, closure, fixer
        micro.time_step(c, 1.0)
        out[key] = (fields(c), micro, c.get_dz())
    off, on = out["off"][0], out["on"][0]
    want = ref.closure(flat3(host(off["temp"]), 1), flat3(host(off["density_dry"]), 1), flat3(host(off["water_vapor"]), 1), flat3(state["temp"], 1),
                       flat3(state["water_vapor"], 1), out["off"][2], 1.0, [0], [0], 0.0)
    assert want["closed_cells"].any() and same_bits(flat3(host(on["temp"]), 1), want["temp"])
    for n in ALL8 + ("precl",):
        if n != "temp":
            assert same_bits(host(on[n]), host(off[n])), n
    got = out["on"][1].heat_closure_stats()
    assert got["cells_closed"] == int(want["counts"][0, 0]) and got["cells_skipped"] == 0
    assert got["residual_K"]["max"] == float(want["max_r"][0]) and got["heating_W_m2"]["max"] == float(want["max_h"][0])
    assert out["off"][1].heat_closure_stats() is None
    assert same_bits(host(out["both"][0]["temp"]), host(on["temp"]))
    for n in WATER + ("precl",):
        assert same_bits(host(out["both"][0][n]), host(out["fix"][0][n])), n
    micro = modules.Microphysics_Kessler_Surrogate()
    c = make_coupler(nz, ny, nx, nens, micro)
    load(c, state)
    micro.heat_closure = True
    with pytest.raises(modules.MWError, match="heat_closure needs online = True"):
        micro.time_step(c, 1.0)
    micro.online, micro.heat_closure = True, {"closed": [0]}
    with pytest.raises(modules.MWError, match="only key is tolerance"):
        micro.time_step(c, 1.0)


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------------
def test_driver_heat_closure(mw, tmp_path, monkeypatch):
    """rollout_surrogates on the 16 x 12 x 10 grid with one constant model listed twice, one copy closed: the JSON carries the block in its
    documented shape; the Kessler member's residual is within the production bound; the closed twin's heating is the reference's, from the
    fields every call was given.  Without the key the document has no such block."""
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver, modules, rollout, surrogate_train as st
    net = water_maker(5, 0.0)                                                   # (all vapour condenses at once: some 30 K at the ground, which the dycore carries)
    paths = st.write_outputs(str(tmp_path / "maker"), np.concatenate([np.ravel(a) for a in net[:4]]), net[4], net[5], {})
    entry = 'keras_weights_txt: "%s", nn_input_scaling: "%s", nn_output_scaling: "%s"' % tuple(paths)
    extra = "surrogate_models:\n  - {name: free, %s}\n  - {name: closed, %s}\npersistence_member: false\n" % (entry, entry)
    seen = []
    real = rollout.heat_closure_finish

    def recording(temp, rho_d, rho_v, before2, nz, ncol, nens, members, closed, tolerance, dz, dt, **kw):
        seen.append(([flat3(host(t), nens) for t in (temp, rho_d, rho_v, before2[0], before2[1])], dz, dt, list(members), list(closed), tolerance))
        return real(temp, rho_d, rho_v, before2, nz, ncol, nens, members, closed, tolerance, dz, dt, **kw)

    monkeypatch.setattr(rollout, "heat_closure_finish", recording)
    docs = {}
    for name, block in (("on", "heat_closure: {closed: [closed], tolerance: 0.0}\n"), ("off", "")):
        d = tmp_path / name
        d.mkdir()
        path, _ = write_yaml(d, nens=3, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra + block)
        monkeypatch.chdir(d)
        coupler, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
        docs[name] = (json.load(open(os.path.join(str(d), "surrogate_rollout.json"))), info, coupler)
    doc, info, coupler = docs["on"]
    assert "heat_closure" not in docs["off"][0] and "heat_closure_report" not in docs["off"][1] and len(seen) == 3
    assert info["heat_closure_report"] == doc["heat_closure"]
    block = doc["heat_closure"]
    assert set(block) == {"lv", "cp_d", "tolerance", "members", "closed", "cells", "columns", "steps", "totals"}
    assert block["lv"] == 2.5e6 and block["cp_d"] == 1003.0 and block["tolerance"] == 0.0 and block["cells"] == 16 * 12 * 10
    assert block["members"] == ["kessler", "free", "closed"] and block["closed"] == ["closed"] and doc["members"] == ["kessler", "free", "closed"]
    assert [s["step"] for s in block["steps"]] == [0, 1, 2]
    kessler = modules.Microphysics_Kessler()
    final = {n: host(t)[..., :1] for n, t in fields(coupler).items()}
    c1 = make_coupler(10, 12, 16, 1, kessler)
    c1.set_grid(8000., 6000., 20000.)
    load(c1, final)
    rs = max(1, kessler.time_step(c1, seen[-1][2], return_rainsplit=True))
    for s, (arrays, dz, dt, members, closed, tol) in zip(block["steps"], seen):
        assert members == [0, 1, 2] and closed == [2] and tol == 0.0
        want = ref.closure(*arrays, dz, dt, members, closed, tol)
        order = ref.kernel_order_stats(want["lanes"])
        assert list(s["members"]) == ["kessler", "free", "closed"]
        for e, n in enumerate(block["members"]):
            row = s["members"][n]
            assert set(row) == {"cells_closed", "cells_skipped", "residual_K", "heating_W_m2"}
            assert set(row["residual_K"]) == {"bias", "mae", "rmse", "max"} and set(row["heating_W_m2"]) == {"mean", "max"}
            print("driver step %d %s: %s (reference counts %s)" % (s["step"], n, json.dumps(row), want["counts"][e].tolist()))
            assert row["cells_closed"] == int(want["counts"][e, 0]) and row["cells_skipped"] == int(want["counts"][e, 1]) == 0
            assert row["heating_W_m2"] == {"mean": float(order[e, 4]) / (16 * 12), "max": float(order[e, 5])}
            assert row["residual_K"]["max"] == float(order[e, 3]) and row["residual_K"]["mae"] == float(order[e, 1]) / (16 * 12 * 10)
        assert s["members"]["closed"]["cells_closed"] > 0 and s["members"]["free"]["cells_closed"] == 0
        bound = 2 * ref.kessler_bound(rs, arrays[0][..., 0]).max()
        print("driver step %d: kessler residual max %.3g K (bound %.3g, rainsplit %d), closed twin heating mean %.3g max %.3g W/m2"
              % (s["step"], s["members"]["kessler"]["residual_K"]["max"], bound, rs, s["members"]["closed"]["heating_W_m2"]["mean"],
                 s["members"]["closed"]["heating_W_m2"]["max"]))
        assert s["members"]["kessler"]["residual_K"]["max"] <= bound
    assert block["totals"]["closed"]["cells_closed"] == sum(s["members"]["closed"]["cells_closed"] for s in block["steps"])
    assert block["totals"]["kessler"]["residual_K"]["max"] == max(s["members"]["kessler"]["residual_K"]["max"] for s in block["steps"])
    skip = ("heat_closure", "yaml", "report", "history", "diverged_at")
    assert {k: v for k, v in doc.items() if k not in skip} == {k: v for k, v in docs["off"][0].items() if k not in skip}
