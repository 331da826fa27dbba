"""The column kernels (csrc/mw_column.hip) through the C ABI at the sizes where their indexing branches, against numpy restatements.

  k_hsum_partial / k_hsum_finish   a slice of SLICE = 16384 cells is summed by four chains that stride 1024 with a tail loop of stride 256
                                   behind them; the slices' partial sums are added in index order
  k_sponge_apply                   1024 elements of ncell_lev * nens per block, the targets of members below 64 cached
  k_nudge_apply                    256 * NUDGE_NPT = 2048 cells per block

No dycore and no oracle: a capi.Grid filled in by hand, plain torch tensors, no all-reduce callback.

Exact inputs.  Every field value is k * 2**-10 with a random nonzero integer |k| <= 2**20 (exact_ints).  Any sum of up to 2**16 such
values is below 2**36 * 2**-10 in magnitude with a spacing of 2**-10: it is exact in fp64 in EVERY association order.  The expected
horizontal sum is therefore integer arithmetic, and every comparison of a sum or a mean below is equality of bits -- a dropped, doubled
or mis-strided cell changes the result, a different summation order does not.

Guard zones.  Every buffer a kernel writes, the workspace (mw_column_workspace_bytes, exactly) included, has TAIL = 4096 sentinel doubles
behind the size the API asks for; they must come back bit for bit (Guarded).

Tolerances: none for sums, means and the nudger.  The sponge's factor holds a cosine: bit for bit where util.host_libm_matches_restatement()
holds, else within 4e-16 * max(1, max|a|) (the rule of test_gpu_simple_city.py for a glibc-cos weight).  The one real-valued sum is held to
math.fsum within (n - 1) * 2**-53 * sum(|x|), the first-order bound of recursive summation in any order.

The shape lists and the restatements are module-level and need numpy only: tests/test_column_edges_cpu.py imports them, checks that the
lists still straddle the kernels' constants, and checks the restatements by hand."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ---- the shapes ---------------------------------------------------------------------------------------------------------------------------
L_TAIL = (1, 63, 64, 65, 255, 256, 257, 768)                      # cells per level: the tail loop alone
L_CHAINS = (769, 1023, 1024, 1025, 1793, 2048)                    # the four-chain loop is entered; every kind of tail behind it
L_SLICES = (16383, 16384, 16385, 16384 + 769, 32768, 32769)       # slice edges
SHAPE_3D = (145, 113)                                             # (ny, nx) with ny * nx = 16385: only the product matters
AVERAGE_SHAPES = [(1, n) for n in L_TAIL + L_CHAINS + L_SLICES] + [SHAPE_3D]
AVERAGE_NENS = (1, 3)
REAL_SUM_L = 32769

SPONGE_NZ = (10, 11, 13)
SPONGE_CASES = ((1023, 1), (1024, 1), (1025, 1), (341, 3), (342, 3), (16385, 1), (300, 63), (300, 64), (300, 65), (300, 130))    # (L, nens)
SPONGE_FIELDS, SPONGE_LAYERS, WFLD = 8, 10, 3                     # 5 + 3 tracers; sponge_layer.h:21,23
SPONGE_DT, SPONGE_TIME_SCALE = 0.7, 60.0

NUDGE_L = (255, 256, 257, 2047, 2048, 2049, 4097)
NUDGE_NENS = (1, 2, 3)
NUDGE_DT, NUDGE_TIME_SCALE = 5.0, 900.0                           # column_nudging.h:62

TAIL = 4096                                                       # sentinel doubles behind every buffer a kernel writes
SENTINEL = -777.25
GRID_SCALE, KMAX = 2.0 ** -10, 2 ** 20


# ---- exact inputs -------------------------------------------------------------------------------------------------------------------------
def exact_ints(seed, shape):
    """Random nonzero int64 k with |k| <= 2**20, one draw per element (so per field, level, cell and member)."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, KMAX, size=shape, endpoint=True) * rng.choice(np.array([-1, 1], dtype=np.int64), size=shape)


def exact_values(ints):
    return ints.astype(np.float64) * GRID_SCALE


def exact_sums(ints, axis):
    """The sum of exact_values(ints) over `axis`, in integers: exact, whatever the order."""
    return ints.sum(axis=axis, dtype=np.int64).astype(np.float64) * GRID_SCALE


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
def column_average_ref(ints, nx_glob, ny_glob):
    """column_nudging.h:80-103 on ints (5, nz, ncell, nens): the sum over the level divided by the GLOBAL cell count (an int product)."""
    return exact_sums(ints, 2) / float(int(nx_glob) * int(ny_glob))


def sponge_factor(k, nz, zlen, dt, time_scale):
    """sponge_layer.h:65,71-74."""
    dz = zlen / nz
    time_factor = dt / time_scale
    z = (k + 0.5) * dz
    rel_dist = (zlen - z) / (SPONGE_LAYERS * dz)
    space_factor = (math.cos(math.pi * rel_dist) + 1) / 2
    return space_factor * time_factor


def sponge_ref(fields, sums, zlen, dt, time_scale, nglob):
    """sponge_layer.h:66-76 on fields (nf, nz, ncell, nens): v + (target - v) * factor on the top ten levels, target = the level's sum over
    all ranks / (nx_glob * ny_glob), 0 for wvel (:50).  sums (nf, 10, nens): the sums of level nz - 1 - kloc; wvel's row is not read."""
    nf, nz = fields.shape[:2]
    out = fields.copy()
    for kloc in range(SPONGE_LAYERS):
        k = nz - 1 - kloc
        factor = sponge_factor(k, nz, zlen, dt, time_scale)
        for f in range(nf):
            target = (np.zeros_like(sums[f, kloc]) if f == WFLD else sums[f, kloc]) / float(nglob)
            v = fields[f, k]
            out[f, k] = v + (target[None, :] - v) * factor
    return out


def nudge_ref(state, column, avg, dt):
    """column_nudging.h:62-65 on state (5, nz, ncell, nens), column and avg (5, nz, nens): q + dt * (column - avg) / 900."""
    inc = dt * (column - avg) / NUDGE_TIME_SCALE
    return state + inc[:, :, None, :]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def close_or_same(got, want):
    """Bit for bit where the host's libm is the build the kernels restate; else 4e-16 * max(1, max|a|)."""
    from util import host_libm_matches_restatement
    if host_libm_matches_restatement():
        return same_bits(got, want)
    return bool(np.all(np.isfinite(got)) and np.max(np.abs(got - want)) <= 4e-16 * max(1.0, float(np.max(np.abs(want)))))


# ---- device buffers and the library calls -------------------------------------------------------------------------------------------------
class Guarded:
    """n elements of `dtype` on the device followed by TAIL sentinel doubles; the elements start out as sentinel bytes too, or as `fill`."""

    def __init__(self, n, dtype=None, fill=None):
        import torch
        dtype = dtype or torch.float64
        self.nbytes = int(n) * torch.empty((), dtype=dtype).element_size()
        words = (self.nbytes + 7) // 8 + TAIL
        self.big = torch.empty(words * 8, dtype=torch.uint8, device="cuda")
        self.big.view(torch.float64).fill_(SENTINEL)
        self.inner = self.big[:self.nbytes].view(dtype)
        self.pattern = np.full(words, SENTINEL).view(np.uint8)[self.nbytes:]
        if fill is not None:
            self.inner.copy_(torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))
        self.ptr = C.c_void_p(self.inner.data_ptr())

    def tail_intact(self):
        return np.array_equal(self.big[self.nbytes:].cpu().numpy(), self.pattern)

    def host(self, shape=None):
        a = self.inner.cpu().numpy()
        return a if shape is None else a.reshape(shape)


def ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*[p.value if isinstance(p, C.c_void_p) else int(p) for p in ptrs])


def make_grid(nz, ny, nx, nens, nx_glob=None, ny_glob=None, zlen=20000.0, px=0, py=0, nproc_x=1, nproc_y=1):
    from miniweatherml_amd import capi
    g = capi.Grid()
    g.nz, g.ny, g.nx, g.nens = nz, ny, nx, nens
    g.nx_glob, g.ny_glob = (nx if nx_glob is None else nx_glob), (ny if ny_glob is None else ny_glob)
    g.zlen = zlen
    g.px, g.py, g.nproc_x, g.nproc_y = px, py, nproc_x, nproc_y
    return g


def column_workspace(g, num_fields):
    from miniweatherml_amd import capi
    nbytes = capi.lib().mw_column_workspace_bytes(C.byref(g), num_fields)
    assert nbytes > 0 and nbytes % 8 == 0
    return Guarded(nbytes // 8)


def no_allreduce():
    """The NULL all-reduce callback: one rank."""
    from miniweatherml_amd import capi
    return C.cast(None, capi.ALLREDUCE_FN)


def set_strict(strict):
    from miniweatherml_amd import capi
    capi.check(capi.lib().mw_column_set_strict(int(strict)))


def column_average(g, fields):
    """mw_column_average on fields (5, nz, ncell, nens): the (5, nz, nens) result; the output's and the workspace's tails are checked."""
    import torch
    from miniweatherml_amd import capi
    dev = [torch.from_numpy(np.ascontiguousarray(fields[f])).cuda() for f in range(5)]
    out, ws = Guarded(5 * g.nz * g.nens), column_workspace(g, 5)
    capi.check(capi.lib().mw_column_average(C.byref(g), ptr_array([t.data_ptr() for t in dev]), out.ptr, ws.ptr, no_allreduce(), None, None))
    torch.cuda.synchronize()
    assert out.tail_intact() and ws.tail_intact(), "column_average wrote behind a buffer"
    for f in range(5):
        assert same_bits(dev[f].cpu().numpy(), fields[f]), "column_average changed its input"
    return out.host((5, g.nz, g.nens))


# ---- mw_column_average --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nens", AVERAGE_NENS)
@pytest.mark.parametrize("shape", AVERAGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_column_average_is_the_exact_sum_over_the_cell_count(mw, shape, nens):
    """Default (sliced four-chain tree) and strict (serial) sums: both are the integer sum's bits, at every tail, chain and slice edge."""
    ny, nx = shape
    nz = 3
    ints = exact_ints([1, ny, nx, nens], (5, nz, ny * nx, nens))
    want = column_average_ref(ints, nx, ny)
    g = make_grid(nz, ny, nx, nens)
    try:
        for strict in (0, 1):
            set_strict(strict)
            got = column_average(g, exact_values(ints))
            bad = np.argwhere(got != want)
            assert same_bits(got, want), "strict %d: %d of %d means differ, first at (field, level, member) %s" % (strict, len(bad), want.size, bad[:1])
    finally:
        set_strict(0)


def test_column_average_divides_by_the_global_count(mw):
    """nx_glob = 2 nx on one rank (no all-reduce): the divisor is nx_glob * ny_glob, not the local cell count."""
    nz, nx, nens = 3, 1025, 3
    ints = exact_ints([2, nx], (5, nz, nx, nens))
    want = column_average_ref(ints, 2 * nx, 1)
    assert not same_bits(want, column_average_ref(ints, nx, 1))
    try:
        for strict in (0, 1):
            set_strict(strict)
            assert same_bits(column_average(make_grid(nz, 1, nx, nens, nx_glob=2 * nx), exact_values(ints)), want), strict
    finally:
        set_strict(0)


def test_real_valued_sums_are_within_the_bound_of_any_order(mw):
    """Normally distributed values of mixed sign at L = 32769 (three slices, the last of one cell).  nx_glob = ny_glob = 1 makes the divisor 1,
    so the output IS the sum.  |sum - fsum| <= (n - 1) 2**-53 sum|x|: the first-order bound of n - 1 rounded additions in any order."""
    nz, nx, nens = 3, REAL_SUM_L, 3
    x = np.random.default_rng(3).normal(size=(5, nz, nx, nens)) * 300.0
    assert (x > 0).any() and (x < 0).any()
    exact = np.array([[[math.fsum(x[f, k, :, e]) for e in range(nens)] for k in range(nz)] for f in range(5)])
    bound = (nx - 1) * 2.0 ** -53 * np.abs(x).sum(axis=2)
    try:
        for strict in (0, 1):
            set_strict(strict)
            got = column_average(make_grid(nz, 1, nx, nens, nx_glob=1, ny_glob=1), x)
            err = np.abs(got - exact)
            print("strict %d: worst |sum - fsum| / bound = %.3e" % (strict, float(np.max(err / bound))))
            assert np.all(np.isfinite(got)) and np.all(err <= bound), strict
    finally:
        set_strict(0)


# ---- mw_sponge_layer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", SPONGE_NZ)
@pytest.mark.parametrize("case", SPONGE_CASES, ids=lambda c: "L%d-nens%d" % c)
def test_sponge_layer_at_block_and_member_edges(mw, case, nz):
    """Eight fields whose members all differ; wvel is all positive (a nonzero mean) and still relaxes towards exactly 0."""
    from miniweatherml_amd import capi
    import torch
    ncell, nens = case
    zlen = 20000.0
    ints = exact_ints([4, ncell, nens, nz], (SPONGE_FIELDS, nz, ncell, nens))
    ints[WFLD] = np.abs(ints[WFLD])
    fields = exact_values(ints)
    sums = exact_sums(ints, 2)[:, ::-1][:, :SPONGE_LAYERS]                        # (nf, kloc, nens): level nz - 1 - kloc
    assert np.all(sums[WFLD] > 0) and (nens == 1 or len(np.unique(sums[0, 0])) == nens)
    want = sponge_ref(fields, sums, zlen, SPONGE_DT, SPONGE_TIME_SCALE, ncell)
    assert np.all(np.abs(want[WFLD, nz - 1]) < np.abs(fields[WFLD, nz - 1]))         # towards 0, not towards its mean of about 512
    g = make_grid(nz, 1, ncell, nens, zlen=zlen)
    bufs = [Guarded(nz * ncell * nens, fill=fields[f]) for f in range(SPONGE_FIELDS)]
    ws = column_workspace(g, SPONGE_FIELDS)
    capi.check(capi.lib().mw_sponge_layer(C.byref(g), ptr_array([b.ptr for b in bufs]), SPONGE_FIELDS, SPONGE_DT, SPONGE_TIME_SCALE, ws.ptr,
                                          no_allreduce(), None, None))
    torch.cuda.synchronize()
    assert ws.tail_intact(), "the workspace's tail was written"
    for f, b in enumerate(bufs):
        assert b.tail_intact(), "field %d: the tail was written" % f
        got = b.host((nz, ncell, nens))
        assert same_bits(got[:nz - SPONGE_LAYERS], fields[f, :nz - SPONGE_LAYERS]), "field %d: a level below the sponge changed" % f
        bad = np.argwhere(got != want[f])
        assert close_or_same(got, want[f]), "field %d: %d cells differ, first at (level, cell, member) %s" % (f, len(bad), bad[:1])


# ---- mw_nudge_to_column -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nens", NUDGE_NENS)
@pytest.mark.parametrize("ncell", NUDGE_L)
def test_nudge_to_column_at_block_edges(mw, ncell, nens):
    """avg is exact and there is no transcendental: q + dt (column - avg) / 900 in numpy, bit for bit.  A sixth field that is passed nowhere
    and the column itself come back unchanged."""
    from miniweatherml_amd import capi
    import torch
    nz = 3
    ints = exact_ints([5, ncell, nens], (6, nz, ncell, nens))
    state = exact_values(ints)
    column = exact_values(exact_ints([6, ncell, nens], (5, nz, nens)))
    avg = column_average_ref(ints[:5], ncell, 1)
    want = nudge_ref(state[:5], column, avg, NUDGE_DT)
    assert np.all(want != state[:5])
    g = make_grid(nz, 1, ncell, nens)
    bufs = [Guarded(nz * ncell * nens, fill=state[f]) for f in range(6)]
    col = torch.from_numpy(column).cuda()
    ws = column_workspace(g, 5)
    capi.check(capi.lib().mw_nudge_to_column(C.byref(g), ptr_array([b.ptr for b in bufs[:5]]), C.c_void_p(col.data_ptr()), NUDGE_DT, ws.ptr,
                                             no_allreduce(), None, None))
    torch.cuda.synchronize()
    assert ws.tail_intact(), "the workspace's tail was written"
    assert same_bits(col.cpu().numpy(), column), "the column changed"
    assert bufs[5].tail_intact() and same_bits(bufs[5].host((nz, ncell, nens)), state[5]), "a field that was not passed changed"
    for f in range(5):
        assert bufs[f].tail_intact(), "field %d: the tail was written" % f
        got = bufs[f].host((nz, ncell, nens))
        bad = np.argwhere(got != want[f])
        assert same_bits(got, want[f]), "field %d: %d cells differ, first at (level, cell, member) %s" % (f, len(bad), bad[:1])
