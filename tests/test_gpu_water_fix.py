"""The water fixer on the GPU: mw_member_water_fix against the numpy statement of its rule (water_fix_ref.py) bit for
bit, the tolerance edge, the order-free and the random sum of the excess, the empty list against mw_member_surface_rain, the entry
checks, the rollout step, the online surrogate and the rollout_surrogates driver.

"Equal in bits" is equality of the int64 views of fp64 arrays; where a planted NaN reaches precl or rain_total, `same` asks for a NaN in
the same place and for equal bits everywhere else (IEEE 754 leaves a NaN's sign and payload open: the GPU negates an operand of a
subtraction with a modifier that flips a NaN's sign, numpy's subtraction keeps it).  Every buffer the call writes -- the three water fields, precl, rain_total,
the workspace (mw_member_water_fix_workspace_bytes, exactly), counts, stats and the excess plane -- has TAIL sentinel doubles behind it
that must come back untouched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import water_fix_ref as ref
from test_gpu_surface_rain import STEP_CASES, GUARD, WATER, bits, host, host_water, same_bits, water_of
from test_gpu_surrogate_rollout import ALL8, fields, load, make_coupler, make_state, model_list, nets

pytestmark = pytest.mark.gpu

TAIL = 4096
SENTINEL = -777.25
DZ = 137.5
HI = (2.0e-2, 2.0e-3, 5.0e-3)                                       # the size of water_vapor, cloud_liquid, precip_liquid


class Guarded:
    """A host fp64 or int64 array on the device with TAIL sentinel doubles behind it."""

    def __init__(self, a):
        import torch
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float64, np.int64)
        self.n, self.dtype = a.size, a.dtype
        self.big = torch.full((a.size + TAIL,), SENTINEL, dtype=torch.float64, device="cuda")
        self.big[:a.size].copy_(torch.from_numpy(a.reshape(-1).view(np.float64)))
        self.shape = a.shape

    @property
    def ptr(self):
        return C.c_void_p(self.big.data_ptr())

    def host(self):
        return self.big[:self.n].cpu().numpy().view(self.dtype).reshape(self.shape).copy()

    def tail_clean(self):
        return bool((self.big[self.n:] == SENTINEL).all())


def same(a, b):
    """NaN where NaN, the same bits everywhere else."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(bits(a)[ok], bits(b)[ok])


def ints(v):
    return (C.c_int * max(1, len(v)))(*[int(x) for x in v])


def call_fix(after, wb, precl0, total0, members, accum, fixed, tol, dz, dt, with_excess=True):
    """mw_member_water_fix on guarded copies of host arrays: a dict of what every buffer holds afterwards."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    nz, ncol, nens = after[0].shape
    w3 = [Guarded(q) for q in after]
    b = {"precl": Guarded(precl0), "rain_total": Guarded(total0), "w_before": Guarded(wb),
         "counts": Guarded(np.full((nens, 2), -5, dtype=np.int64)), "stats": Guarded(np.full((nens, 2), SENTINEL)),
         "excess": Guarded(np.full((ncol, nens), SENTINEL))}
    nbytes = L.mw_member_water_fix_workspace_bytes(ncol, nens)
    assert nbytes == ((ncol * nens + 255) // 256) * nens * 32
    ws = Guarded(np.full(nbytes // 8, SENTINEL))
    ptrs = (C.c_void_p * 3)(*[w.ptr.value for w in w3])
    capi.check(L.mw_member_water_fix(nz, ncol, nens, len(members), ints(members), len(accum), ints(accum), len(fixed), ints(fixed), float(tol),
                                     ptrs, float(dz), float(dt), b["w_before"].ptr, b["precl"].ptr, b["rain_total"].ptr, ws.ptr,
                                     b["counts"].ptr, b["stats"].ptr, b["excess"].ptr if with_excess else None, None))
    torch.cuda.synchronize()
    for g in w3 + list(b.values()) + [ws]:
        assert g.tail_clean()
    out = {k: g.host() for k, g in b.items()}
    out.update(v=w3[0].host(), c=w3[1].host(), r=w3[2].host())
    assert same_bits(out["w_before"], wb)
    return out


def lists_for(nens):
    """(members, accum, fixed): the last member and member 0 fixed, one budget member that is not, every member accumulated (four of 64)."""
    fixed = [nens - 1] + ([0] if nens > 2 else [])
    extra = [e for e in range(nens) if e not in fixed][:1]
    accum = [0, 63, 5, 17] if nens == 64 else list(range(nens))
    return fixed + extra, accum, fixed


def recipe(nz, ncol, nens, seed):
    """(after, w_before, planted): non-negative fields before, after = before * a per-column factor in [0.5, 1.5] + per-cell noise, and,
    where the plane has room, the planted cases on fixed members: W_b = 0 with W_a > 0, W_a == W_b, W_b < 0, a NaN cell, an inf cell; the
    second wavefront of the plane with no column to fix and the third with one."""
    rng = np.random.default_rng(seed)
    _, _, fixed = lists_for(nens)
    plane = ncol * nens
    before = [rng.uniform(0.0, hi, (nz, ncol, nens)) for hi in HI]
    factor = rng.uniform(0.5, 1.5, plane)
    planted = {}
    if plane >= 128:
        factor[64:128] = 0.6
    if plane >= 192:
        factor[128:192] = 0.6
        planted["lone"] = next(t for t in range(128, 192) if t % nens in fixed)
        factor[planted["lone"]] = 1.4
    factor = factor.reshape(ncol, nens)
    pairs = [(c, e) for c in range(ncol) for e in fixed][::-1]
    if len(pairs) >= 10:
        planted.update(zip(("zero", "equal", "negative", "nan", "inf"), pairs))
        for q in before:
            q[:, planted["zero"][0], planted["zero"][1]] = 0.0
        factor[planted["equal"]] = 1.0
    after = [q * factor + rng.uniform(0.0, 1.0e-3 * hi, q.shape) for q, hi in zip(before, HI)]
    wb = ref.column_water(*before, DZ)
    if "equal" in planted:
        c, e = planted["equal"]
        for q, b in zip(after, before):
            q[:, c, e] = b[:, c, e]
        wb[planted["negative"]] = -1.0
        after[1][nz // 2, planted["nan"][0], planted["nan"][1]] = np.nan
        after[2][nz - 1, planted["inf"][0], planted["inf"][1]] = np.inf
    return after, wb, planted


def grid_recipe(nz, ncol, nens, dz, seed, last_gains=False):
    """(after, w_before) on the 2^-10 grid (dz a power of two): every W and every partial sum of the excess is exact.  last_gains: every
    cell of the last column gains 2^-4, eight times what any other cell can."""
    rng = np.random.default_rng(seed)
    before = [rng.integers(0, 64, (nz, ncol, nens)) / 1024.0 for _ in range(3)]
    after = [q + rng.integers(-8, 9, q.shape).clip(-q * 1024.0, None) / 1024.0 for q in before]
    if last_gains:
        for q, b in zip(after, before):
            q[:, -1] = b[:, -1] + 0.0625
    return after, ref.column_water(*before, dz)


# the last shape: 65,538 plane elements are 257 blocks, the smallest plane at which a thread of the final kernel (thread 0: block rows 0
# and 256) folds two rows; five levels are one look-ahead group and a tail.  Its fields are grid_recipe's, so the sum is held exactly,
# and its last column (of block 256) gains the most: row 256 carries a count, a part of the sum and the maximum of the last member.
STRIDE = (5, 21846, 3)
SHAPES = [(1, 1, 1), (2, 1, 3), (3, 65, 2), (4, 64, 4), (5, 7, 64), (8, 255, 1), (9, 64, 4), (9, 257, 1), (37, 257, 3), STRIDE]
_CASES = {}


def dz_of(shape):
    return 128.0 if shape == STRIDE else DZ


def case(shape):
    """The recipe, the call's result and the reference's for a shape, computed once and never changed."""
    if shape not in _CASES:
        nz, ncol, nens = shape
        if shape == STRIDE:
            (after, wb), planted = grid_recipe(nz, ncol, nens, dz_of(shape), seed=sum(shape), last_gains=True), {}
        else:
            after, wb, planted = recipe(nz, ncol, nens, seed=sum(shape))
        members, accum, fixed = lists_for(nens)
        rng = np.random.default_rng(7)
        precl0, total0 = rng.uniform(1.0, 2.0, (ncol, nens)), rng.uniform(-1.0, 1.0, (ncol, nens))
        dt = 0.5 if nz % 2 else 60.0
        got = call_fix(after, wb, precl0, total0, members, accum, fixed, 0.0, dz_of(shape), dt)
        want = ref.water_fix(*after, dz_of(shape), dt, wb, precl0, total0, members, accum, fixed, 0.0)
        _CASES[shape] = (after, wb, planted, got, want, (members, accum, fixed))
    return _CASES[shape]


# ---- 1. the kernel against the rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_bit_for_bit(mw, shape):
    """nz below, at and above the look-ahead of four and its multiples; planes below, at and above a wavefront and a block; bit 63 of the
    member mask; 257 blocks (STRIDE), where the sum is the reference's bits too.  The three fields, precl, rain_total, the excess plane,
    both counts and the maximum are the reference's bits; a later mw_member_column_water returns the W' that precl was made of."""
    import torch
    from miniweatherml_amd import microphysics
    nz, ncol, nens = shape
    after, wb, planted, got, want, (members, accum, fixed) = case(shape)
    for k in ("v", "c", "r", "excess"):
        assert same_bits(got[k], want[k]), k
    for k in ("precl", "rain_total"):
        assert same(got[k], want[k]), k
    assert np.array_equal(got["counts"], want["counts"])
    assert same_bits(got["stats"][:, 1], want["max"])
    unfixed = [e for e in range(nens) if e not in fixed]
    assert np.all(got["counts"][unfixed] == 0) and np.all(bits(got["stats"][unfixed]) == 0)
    fix = want["fixed"]
    if ncol * nens >= 64:
        assert fix.any() and not fix[:, fixed].all()
    flat = fix.reshape(-1)
    if "lone" in planted:
        assert not flat[64:128].any() and list(np.flatnonzero(flat[128:192]) + 128) == [planted["lone"]]
    if "zero" in planted:
        assert fix[planted["zero"]] and all(np.all(got[k][:, planted["zero"][0], planted["zero"][1]] == 0.0) for k in "vcr")
        assert not fix[planted["equal"]] and bits(got["precl"][planted["equal"]]) == 0
        for name in ("negative", "nan", "inf"):
            assert want["skipped"][planted[name]] and not fix[planted[name]], name
        assert int(want["counts"][:, 1].sum()) == 3
    # the bound on the residual, and the state's own column water
    w3 = [torch.from_numpy(got[k]).cuda() for k in "vcr"]
    w_now = host(microphysics.column_water(w3, nz, ncol, nens, dz_of(shape))).reshape(ncol, nens)
    assert same(w_now, want["w_now"])
    live = fix & (wb > 0.0)
    if live.any():
        print("residual %s: largest |W' - W_b| = %.3g units of 2^-52 W_b, bound %d"
              % ("x".join(map(str, shape)), float(np.max(np.abs(w_now[live] - wb[live]) / (2.0 ** -52 * wb[live]))), nz + 4))
    assert np.all(np.abs(w_now[fix] - wb[fix]) <= ref.bound(nz, wb[fix]))
    # the sum of the excess: the kernels' order against numpy's, within n * 2^-52 * sum |x| (k_surrogate_sums' yardstick)
    assert np.all(np.abs(got["stats"][:, 0] - want["sum"]) <= ncol * 2.0 ** -52 * np.abs(want["excess"]).sum(axis=0))
    if shape == STRIDE:                                                         # every order agrees: the second turn of the final kernel's loop too
        assert same_bits(got["stats"][:, 0], want["sum"]) and np.all(want["counts"][fixed, 0] > 256)
        assert fix[-1, nens - 1] and want["excess"][-1, nens - 1] == want["max"][nens - 1] == dz_of(shape) * nz * 3 * 0.0625
        assert np.all(want["sum"] == np.array([float(np.sum(want["excess"][::-1, e])) for e in range(nens)]))      # (exact indeed)
    # members in no list keep every bit; without the excess plane nothing else changes
    idle = [e for e in range(nens) if e not in members and e not in accum]
    rng = np.random.default_rng(7)
    precl0 = rng.uniform(1.0, 2.0, (ncol, nens))
    assert same_bits(got["precl"][:, idle], precl0[:, idle]) and np.all(bits(got["excess"][:, idle]) == 0)


def test_without_the_excess_plane(mw):
    shape = (9, 64, 4)
    after, wb, _, got, _, (members, accum, fixed) = case(shape)
    rng = np.random.default_rng(7)
    precl0, total0 = rng.uniform(1.0, 2.0, (64, 4)), rng.uniform(-1.0, 1.0, (64, 4))
    bare = call_fix(after, wb, precl0, total0, members, accum, fixed, 0.0, DZ, 0.5, with_excess=False)
    for k in ("v", "c", "r", "precl", "rain_total", "counts", "stats"):
        assert same_bits(bare[k].view(np.float64), got[k].view(np.float64)), k
    assert np.all(bare["excess"] == SENTINEL)


def test_tolerance_edge(mw):
    """dz = 1, W_b = 1, W_a = (1 + 0.25) + 0.25 = 1.5: the excess 0.5 is not greater than 0.5 * W_b; it is greater than the next fp64
    below 0.5 times W_b."""
    one = [np.full((1, 1, 1), x) for x in (1.0, 0.25, 0.25)]
    args = (np.ones((1, 1)), np.full((1, 1), 9.0), np.zeros((1, 1)), [0], [0], [0])
    kept = call_fix(one, *args, 0.5, 1.0, 1.0)
    assert kept["counts"].tolist() == [[0, 0]] and all(same_bits(kept[k], q) for k, q in zip("vcr", one))
    assert kept["precl"][0, 0] == -0.5 / 1000.0 and bits(kept["excess"])[0, 0] == 0 and np.all(bits(kept["stats"]) == 0)
    tol = float(np.nextafter(0.5, 0.0))
    fixed = call_fix(one, *args, tol, 1.0, 1.0)
    want = ref.water_fix(*one, 1.0, 1.0, *args, tol)
    assert fixed["counts"].tolist() == [[1, 0]] and fixed["excess"][0, 0] == 0.5 and fixed["stats"].tolist() == [[0.5, 0.5]]
    for k in ("v", "c", "r", "precl", "rain_total"):
        assert same_bits(fixed[k], want[k]), k
    assert fixed["v"][0, 0, 0] == 1.0 * (1.0 / 1.5)


def test_sum_of_excess_where_every_order_agrees(mw):
    """Fields on a 2^-10 grid and dz a power of two: every W and every partial sum of the excess is exact, so any order of the blocks and
    lanes gives the same bits as numpy's."""
    nz, ncol, nens = 6, 700, 3
    after, wb = grid_recipe(nz, ncol, nens, 128.0, seed=11)
    members = accum = fixed = [2, 0, 1]
    z = np.zeros((ncol, nens))
    got = call_fix(after, wb, z, z, members, accum, fixed, 0.0, 128.0, 1.0)
    want = ref.water_fix(*after, 128.0, 1.0, wb, z, z, members, accum, fixed, 0.0)
    assert np.all(want["counts"][:, 0] > 100) and np.all(want["counts"][:, 0] < ncol - 100)
    assert same_bits(got["excess"], want["excess"]) and np.array_equal(got["counts"], want["counts"])
    assert same_bits(got["stats"][:, 0], want["sum"]) and same_bits(got["stats"][:, 1], want["max"])
    assert np.all(want["sum"] == np.array([float(np.sum(want["excess"][::-1, e])) for e in range(nens)]))      # (exact indeed)


# ---- 2. the empty list and the entry checks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 65, 2), (9, 257, 1), (5, 7, 64)])
def test_empty_fixed_list_is_surface_rain(mw, shape):
    import torch
    from miniweatherml_amd import capi
    nz, ncol, nens = shape
    after, wb, _, _, _, (members, accum, _) = case(shape)
    rng = np.random.default_rng(3)
    precl0, total0 = rng.uniform(1.0, 2.0, (ncol, nens)), rng.uniform(-1.0, 1.0, (ncol, nens))
    got = call_fix(after, wb, precl0, total0, members, accum, [], 0.0, DZ, 60.0)
    w3 = [Guarded(q) for q in after]
    p, t, w = Guarded(precl0), Guarded(total0), Guarded(wb)
    capi.check(capi.lib().mw_member_surface_rain(nz, ncol, nens, len(members), ints(members), len(accum), ints(accum),
                                                 (C.c_void_p * 3)(*[g.ptr.value for g in w3]), DZ, 60.0, w.ptr, p.ptr, t.ptr, None))
    torch.cuda.synchronize()
    assert same(got["precl"], p.host()) and same(got["rain_total"], t.host())
    for k, q in zip("vcr", after):
        assert same_bits(got[k], q), k
    assert np.all(got["counts"] == 0) and np.all(bits(got["stats"]) == 0) and np.all(bits(got["excess"]) == 0)


def test_entry_checks(mw):
    """Every refusal names its reason, launches nothing and leaves every buffer as it was."""
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    nz, ncol, nens = 4, 16, 3
    f = [torch.rand((nz, ncol, nens), dtype=torch.float64, device="cuda") for _ in range(3)]
    f0 = [t.clone() for t in f]
    full = lambda v, n=ncol * nens: torch.full((n,), v, dtype=torch.float64, device="cuda")     # noqa: E731
    wb, precl, total, excess, stats = full(0.001), full(3.0), full(5.0), full(11.0), full(13.0, 2 * nens)
    counts = torch.full((2 * nens,), -1, dtype=torch.int64, device="cuda")
    ws = full(17.0, L.mw_member_water_fix_workspace_bytes(ncol, nens) // 8)
    ptrs = modules._field_ptr_array(f)
    holed = modules._field_ptr_array(f)
    holed[1] = None
    twice = modules._field_ptr_array([f[0], f[1], f[0]])
    P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731

    def fix(nz=nz, ncol=ncol, nens=nens, members=(1, 2), accum=(0, 1, 2), fixed=(1,), tol=0.0, water=ptrs, dz=500.0, dt=1.0, wb=P(wb),
            precl=P(precl), total=P(total), ws=P(ws), counts=P(counts), stats=P(stats), excess=P(excess), nfix=None):
        return L.mw_member_water_fix(nz, ncol, nens, len(members), ints(members), len(accum), ints(accum), len(fixed) if nfix is None else nfix,
                                     ints(fixed), tol, water, dz, dt, wb, precl, total, ws, counts, stats, excess, None)

    nan, inf = float("nan"), float("inf")
    cases = [(lambda: fix(nz=0), "nz and ncol must be >= 1"), (lambda: fix(ncol=0), "nz and ncol must be >= 1"),
             (lambda: fix(nens=0), r"nens must be in \[1, 64\]"), (lambda: fix(nens=65), r"nens must be in \[1, 64\]"),
             (lambda: fix(members=(3,)), r"member 3 is outside \[0, 3\)"), (lambda: fix(accum=(0, -1)), r"member -1 is outside \[0, 3\)"),
             (lambda: fix(fixed=(4,)), r"member 4 is outside \[0, 3\)"),
             (lambda: fix(members=(1, 1)), "member 1 is listed twice in members"), (lambda: fix(accum=(2, 0, 2)), "member 2 is listed twice in accum"),
             (lambda: fix(members=(0, 1, 2), fixed=(1, 2, 1)), "member 1 is listed twice in fixed"),
             (lambda: fix(nfix=4, fixed=(0, 1, 2, 2)), "fixed holds 4 members"), (lambda: fix(nfix=-1), "fixed holds -1 members"),
             (lambda: fix(fixed=(0,)), "member 0 is in fixed but not in members"),
             (lambda: fix(members=(), fixed=(2,), wb=None), "member 2 is in fixed but not in members"),
             (lambda: fix(tol=-1.0e-300), "tolerance must be finite and >= 0"), (lambda: fix(tol=nan), "tolerance must be finite and >= 0"),
             (lambda: fix(tol=inf), "tolerance must be finite and >= 0"),
             (lambda: fix(dt=0.0), "dt must be positive and finite"), (lambda: fix(dt=inf), "dt must be positive and finite"),
             (lambda: fix(dt=nan), "dt must be positive and finite"), (lambda: fix(dz=0.0), "dz must be positive and finite"),
             (lambda: fix(dz=-1.0), "dz must be positive and finite"), (lambda: fix(dz=nan), "dz must be positive and finite"),
             (lambda: fix(dz=inf), "dz must be positive and finite"),
             (lambda: fix(water=None), "null pointer"), (lambda: fix(water=holed), "null field"), (lambda: fix(water=twice), "three arrays"),
             (lambda: fix(wb=None), "null pointer"), (lambda: fix(precl=None), "null pointer"), (lambda: fix(total=None), "null pointer"),
             (lambda: fix(ws=None), "null pointer"), (lambda: fix(counts=None), "null pointer"), (lambda: fix(stats=None), "null pointer")]
    for call, msg in cases:
        with pytest.raises(modules.MWError, match=msg):
            capi.check(call())
    torch.cuda.synchronize()
    assert all(bool((t == v).all()) for t, v in ((precl, 3.0), (total, 5.0), (excess, 11.0), (stats, 13.0), (ws, 17.0), (counts, -1)))
    assert all(torch.equal(a, b) for a, b in zip(f, f0))
    for bad in ((0, 3), (16, 0), (16, 65)):
        assert L.mw_member_water_fix_workspace_bytes(*bad) == 0
    # what is allowed: no excess plane, no rain_total without accum, nothing listed at all (the statistics are still set)
    assert fix(excess=None) == 0 and fix(accum=(), total=None) == 0
    assert fix(members=(), accum=(), fixed=(), wb=None, total=None) == 0
    torch.cuda.synchronize()
    assert bool((counts == 0).all()) and bool((stats == 0.0).all()) and bool((excess == 0.0).all())
    # the wrappers refuse what the kernel cannot be given
    c = make_coupler(nz, 1, ncol, nens, modules.Microphysics_Kessler())
    with pytest.raises(modules.MWError, match="w_before must be"):
        modules.member_water_fix(c, [1], [], [1], 1.0, wb)


# ---- 3. the rollout step -----------------------------------------------------------------------------------------------------------------
def water_maker(n_in, level):
    """A state-form model of the pool's width whose W2 is zero: its outputs are constants, the water fields at `level` of their range."""
    W1, b1, W2, b2, si, so = nets(n_in)[0][:6]
    return (W1, b1, np.zeros_like(W2), np.array([0.5, level, level, level], dtype=np.float32), si, so)


def step_members(micro, listed):
    return [micro.member_names.index(n) for n in listed]


@pytest.mark.parametrize("shape,kind,k,persistence,committee", STEP_CASES,
                         ids=["%s-%s%d-%s-%s" % ("x".join(map(str, s)), kind, k, "pers" if p else "nopers", c) for s, kind, k, p, c in STEP_CASES])
def test_rollout_step(mw, shape, kind, k, persistence, committee):
    """One step without the option and one with it, from a dry state (the constant model makes water in every column) and from a wet one
    (it removes water): a member not listed keeps the first run's bits; a listed member is the reference applied to the first run's state
    of that member and the first run's W_before.  With water_fixer = None and surface_rain the step is the budget's, as before."""
    from miniweatherml_amd import modules
    nz, ny, nx, nens = shape
    models = model_list(kind, k)
    models[0] = water_maker(int(models[0][0].shape[0]), 0.05)
    names = ["m%d" % i for i in range(k)]
    committees = [] if committee is None else [("com", names) + ((GUARD,) if committee == "guarded" else ())]
    listed = ["m0"] + (["com"] if committee else [])
    wet = make_state(shape, seed=sum(shape) + k)
    dry = {n: (0.01 * a if n in WATER else a) for n, a in wet.items()}
    offs = {}
    for label, state in (("dry", dry), ("wet", wet)):
        runs = []
        for option in (None, {"members": listed, "tolerance": 0.0}):
            micro = modules.Microphysics_Rollout()
            c = make_coupler(nz, ny, nx, nens, micro, models=models, persistence=persistence, names=names, committees=committees)
            load(c, state)
            micro.water_fixer = option
            micro.time_step(c, 1.0)
            runs.append((fields(c), micro, c))
        (off, m_off, c_off), (on, m_on, _) = runs
        offs[label] = off
        assert m_off.rain_total is None and m_off.water_fix_reports() is None
        fixed = step_members(m_on, listed)
        dz = c_off.get_dz()
        flat = lambda a: a.reshape(a.shape[0], ny * nx, nens)                   # noqa: E731
        wb = host_water(*[flat(state[n]) for n in WATER], dz)
        want = ref.water_fix(*[flat(host(off[n])) for n in WATER], dz, 1.0, wb, host(off["precl"]).reshape(-1, nens),
                             np.zeros((ny * nx, nens)), fixed, range(nens), fixed, 0.0)
        for n in ALL8:
            if n not in WATER:
                assert same_bits(host(on[n]), host(off[n])), (label, n)          # temp and density_dry among them: a mass fixer
        for n, key in zip(WATER, "vcr"):
            assert same_bits(flat(host(on[n])), want[key]), (label, n)
            rest = [e for e in range(nens) if e not in fixed]
            assert same_bits(host(on[n])[..., rest], host(off[n])[..., rest]), (label, n)
        assert same(host(on["precl"]).reshape(-1, nens), want["precl"]), label
        assert same(host(m_on.rain_total).reshape(-1, nens), want["rain_total"]), label
        m0 = fixed[0]
        if label == "dry":
            assert want["fixed"][:, m0].all()
        else:
            assert not want["fixed"][:, m0].all()
        m_on.water_fix_record(7)
        rep = m_on.water_fix_reports()
        assert rep["members"] == listed and rep["columns"] == ny * nx and [s["step"] for s in rep["steps"]] == [7]
        for n, e in zip(listed, fixed):
            row = rep["steps"][0]["members"][n]
            assert row["columns_fixed"] == int(want["counts"][e, 0]) and row["columns_skipped"] == int(want["counts"][e, 1])
            assert row["water_removed_kg_m2"]["max"] == float(want["max"][e])
    # the fixer beside surface_rain: the budget members are the union; with None the step is surface_rain's
    micro = modules.Microphysics_Rollout()
    c = make_coupler(nz, ny, nx, nens, micro, models=models, persistence=persistence, names=names, committees=committees)
    load(c, dry)
    micro.surface_rain = {}
    micro.time_step(c, 1.0)
    both = modules.Microphysics_Rollout()
    cb = make_coupler(nz, ny, nx, nens, both, models=models, persistence=persistence, names=names, committees=committees)
    load(cb, dry)
    both.surface_rain, both.water_fixer = {}, {"members": ["m0"]}
    both.time_step(cb, 1.0)
    f_sr, f_both = fields(c), fields(cb)
    for n in ALL8:
        assert same_bits(host(f_sr[n]), host(offs["dry"][n])), n
    after = host_water(*water_of(c), c.get_dz())
    wb4 = host_water(*[dry[n] for n in WATER], c.get_dz())
    assert same_bits(host(f_sr["precl"])[..., 1:], ((wb4 - after) / 1000.0)[..., 1:])
    rest = [e for e in range(nens) if e != 1]
    assert same_bits(host(f_both["precl"])[..., rest], host(f_sr["precl"])[..., rest])
    assert np.all(np.abs(host(f_both["precl"])[..., 1]) <= ref.bound(nz, wb4[..., 1]) / 1000.0)
    for bad, msg in (({"member": ["m0"]}, "keys are members and tolerance"), ({"members": ["kessler"]}, "never kessler or persistence"),
                     ({"members": ["m0", "m0"]}, "distinct network-stepped"), ({"tolerance": -1.0}, "finite number >= 0")):
        both.water_fixer = bad
        with pytest.raises(modules.MWError, match=msg):
            both.time_step(cb, 1.0)


# ---- 4. the online surrogate -------------------------------------------------------------------------------------------------------------
def test_online_surrogate_water_fixer(mw):
    """online with water_fixer (a committee of one constant model, which makes water in about half the columns): the state is the
    reference applied to what the network leaves without it, the plane as one member; online = False with the option is refused."""
    from miniweatherml_amd import modules
    shape = (9, 3, 11, 2)
    nz, ny, nx, nens = shape
    state = make_state(shape, seed=sum(shape))
    for n in WATER:                                                             # a column's mean is about the constant the network writes
        state[n] = 0.6 * state[n]
    maker = [water_maker(5, 0.3)]
    out = []
    for option in (None, {"tolerance": 0.0}):
        micro = modules.Microphysics_Kessler_Surrogate()
        c = make_coupler(nz, ny, nx, nens, micro, committee=maker)
        load(c, state)
        micro.online, micro.surface_rain, micro.water_fixer = True, True, option
        micro.time_step(c, 1.0)
        out.append((fields(c), micro, c.get_dz()))
    (off, _, dz), (on, micro_on, _) = out
    flat = lambda a: a.reshape(nz, -1, 1)                                       # noqa: E731
    wb = host_water(*[flat(state[n]) for n in WATER], dz)
    want = ref.water_fix(*[flat(host(off[n])) for n in WATER], dz, 1.0, wb, host(off["precl"]).reshape(-1, 1), np.zeros((ny * nx * nens, 1)),
                         [0], [], [0], 0.0)
    assert want["fixed"].any() and not want["fixed"].all()
    for n, key in zip(WATER, "vcr"):
        assert same_bits(flat(host(on[n])), want[key]), n
    for n in ALL8:
        if n not in WATER:
            assert same_bits(host(on[n]), host(off[n])), n
    assert same(host(on["precl"]).reshape(-1, 1), want["precl"])
    got = micro_on.water_fix_stats()
    assert got["columns_fixed"] == int(want["counts"][0, 0]) and got["columns_skipped"] == 0
    assert got["water_removed_kg_m2"]["max"] == float(want["max"][0])
    micro = modules.Microphysics_Kessler_Surrogate()
    c = make_coupler(nz, ny, nx, nens, micro)
    load(c, state)
    micro.water_fixer = True
    with pytest.raises(modules.MWError, match="water_fixer needs online = True"):
        micro.time_step(c, 1.0)
    micro.online, micro.water_fixer = True, {"members": [0]}
    with pytest.raises(modules.MWError, match="only key is tolerance"):
        micro.time_step(c, 1.0)


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------------
def test_driver_water_fixer(mw, tmp_path, monkeypatch):
    """rollout_surrogates on the 16 x 12 x 10 grid with surface_rain (every member's precl is its water budget) and one water-making model
    listed twice, one copy fixed: the JSON carries the block; the fixed twin's accumulated rain is >= -(the bound summed over the steps,
    from the W_before of every call); the unfixed twin's is negative.  Without the key the document has no such block and both twins
    are the unfixed one."""
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver, rollout, surrogate_train as st
    net = water_maker(5, 0.5)
    paths = st.write_outputs(str(tmp_path / "maker"), np.concatenate([np.ravel(a) for a in net[:4]]), net[4], net[5], {})
    entry = 'keras_weights_txt: "%s", nn_input_scaling: "%s", nn_output_scaling: "%s"' % tuple(paths)
    extra = "surrogate_models:\n  - {name: free, %s}\n  - {name: fixed, %s}\npersistence_member: false\nsurface_rain: {map: false}\n" % (entry, entry)
    seen = []
    real = rollout.water_fix_finish

    def recording(water3, nz, ncol, nens, members, accum, fixed, tolerance, dz, dt, w_before, *a, **kw):
        seen.append(w_before.detach().cpu().numpy().reshape(ncol, nens).copy())
        return real(water3, nz, ncol, nens, members, accum, fixed, tolerance, dz, dt, w_before, *a, **kw)

    monkeypatch.setattr(rollout, "water_fix_finish", recording)
    docs = {}
    for name, block in (("on", "water_fixer: {members: [fixed], tolerance: 0.0}\n"), ("off", "")):
        d = tmp_path / name
        d.mkdir()
        path, _ = write_yaml(d, nens=3, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra + block)
        monkeypatch.chdir(d)
        _, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
        docs[name] = (json.load(open(os.path.join(str(d), "surrogate_rollout.json"))), info)
    doc, info = docs["on"]
    assert "water_fixer" not in docs["off"][0] and "water_fixer_report" not in docs["off"][1] and len(seen) == 3
    skip = ("water_fixer", "surface_rain", "yaml", "report", "history", "diverged_at")
    assert {k: v for k, v in doc.items() if k not in skip} == {k: v for k, v in docs["off"][0].items() if k not in skip}
    assert info["water_fixer_report"] == doc["water_fixer"]
    block = doc["water_fixer"]
    assert block["tolerance"] == 0.0 and block["members"] == ["fixed"] and block["columns"] == 16 * 12
    assert [s["step"] for s in block["steps"]] == [0, 1, 2] and doc["members"] == ["kessler", "free", "fixed"]
    for s in block["steps"]:
        row = s["members"]["fixed"]
        assert list(s["members"]) == ["fixed"] and 0 <= row["columns_fixed"] <= 16 * 12 and row["columns_skipped"] == 0
        assert row["water_removed_kg_m2"]["max"] >= row["water_removed_kg_m2"]["mean"] >= 0.0
    assert block["steps"][0]["members"]["fixed"]["columns_fixed"] > 0
    assert block["totals"]["fixed"]["columns_fixed"] == sum(s["members"]["fixed"]["columns_fixed"] for s in block["steps"])
    total = host(info["rain_total"]).reshape(-1, 3)
    floor = sum(ref.bound(10, np.maximum(w[:, 2], 0.0)) for w in seen) / 1000.0
    print("driver: fixed twin min %.3e (floor %.3e), unfixed twin max %.3e" % (total[:, 2].min(), -floor.max(), total[:, 1].max()))
    assert np.all(total[:, 2] >= -floor)
    assert np.all(total[:, 1] < 0.0)
    unfixed = host(docs["off"][1]["rain_total"]).reshape(-1, 3)
    assert same_bits(unfixed[:, 1], total[:, 1]) and same_bits(unfixed[:, 2], unfixed[:, 1]) and same_bits(unfixed[:, 0], total[:, 0])
