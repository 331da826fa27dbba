"""Option lean_stores (default 1): k_xz_state<.., VAP> leaves out the stores that only FULL iterations of the tracer stage read -- the x and z
mass fluxes and selectors of a level whose row-map words are clear on this tile's and its neighbour tiles' segments, and in the last stage the
result slab's density and pressure slots of a lean cell; a replay launch stores them when the stage's vapour is redone; tracer waves that
leave early leave their zero flag bytes out while the buffer is known to hold zeros.

Every comparison: lean_stores = 1 against lean_stores = 0 on the same state and options, all eight coupler fields bit for bit after each of
three time steps, zero_verify on with no violation.  In front of every step, on both sides, mw_debug_poison_handoff fills everything the kernel may
leave out with NaN / 0xFF.  A reader that consumes a skipped slab slot turns density_dry and temp into NaN; one that consumes a skipped face
turns a tracer's tendency into NaN, which the positivity clip stores as 0 -- the comparison fails wherever the tracer's true value is not 0.
(Where it is 0 the face multiplies an edge value of exactly 0, and no finite face value changes the result: that is the margin the maps keep
round every non-zero cell, and why a library without the neighbour-tile widening of the mask passes these tests -- the widening guards
against a non-finite stale value only.  The control that does fail is a library without the replay launch: test_forced_redo_is_replayed.)

Which faces are left out follows from the seeded box of cloud and rain: the stage-s word of level w is set when cloud or rain is non-zero within
levels w - 3 s - 5 .. w + 3 s + 1, within 3 s rows, in a segment within nine cells.  The first step's maps are read back and the kernel's
predicate is evaluated on them, so a case cannot pass on a state on which nothing was left out, or on which everything was."""
import ctypes as C

import numpy as np
import pytest

from util import gpu_fields, record_comparison

pytestmark = pytest.mark.gpu

TILE = 58                                                        # cells an x/z marching wave completes (WENO-5, one member)
PATH = "march ord5 K1 nens1 one_stream y_all conv_in_y tracers_fused 3d"


def _seed_box(coupler, box):
    """cloud and rain on the cells (k0 .. k1, j0 .. j1, x0 .. x1), smoothly varying and non-zero in every cell of the box"""
    import torch
    k0, k1, j0, j1, x0, x1 = box
    dm = coupler.get_data_manager_readwrite()
    rho = dm.get("density_dry")
    nz, ny, nx = rho.shape[0], rho.shape[1], rho.shape[2]
    k = torch.arange(nz, device=rho.device, dtype=torch.float64).view(nz, 1, 1, 1)
    j = torch.arange(ny, device=rho.device, dtype=torch.float64).view(1, ny, 1, 1)
    i = torch.arange(nx, device=rho.device, dtype=torch.float64).view(1, 1, nx, 1)
    inside = ((k >= k0) & (k <= k1) & (j >= j0) & (j <= j1) & (i >= x0) & (i <= x1)).to(torch.float64)
    dm.get("cloud_liquid").copy_(2.0e-3 * inside * (0.5 + 0.5 * torch.sin(0.3 * k + 0.05 * i) ** 2) * rho)
    dm.get("precip_liquid").copy_(4.0e-4 * inside * (0.5 + 0.5 * torch.cos(0.2 * k + 0.03 * j) ** 2) * rho)


def _seed_rim(coupler):
    """single cloud / rain cells of very different size side by side in row 2, in a strong random wind: their limiter multipliers drop below 1
    and y faces are scaled (the state of tests/test_gpu_vapour_state.py's flag-byte tests)"""
    import torch
    f = gpu_fields(coupler)
    rho = f["density_dry"]
    nz, ny, nx = rho.shape[0], rho.shape[1], rho.shape[2]
    k = np.arange(nz, dtype=np.float64).reshape(nz, 1, 1, 1)
    i = np.arange(nx, dtype=np.float64).reshape(1, 1, nx, 1)
    j = np.arange(ny, dtype=np.float64).reshape(1, ny, 1, 1)
    rng = np.random.default_rng(7)
    for n, amp in (("uvel", 25.0), ("vvel", 25.0), ("wvel", 8.0)):
        f[n] += amp * rng.uniform(-1, 1, f[n].shape)
    speck = (rng.uniform(size=rho.shape) > 0.5) * ((i >= 16) & (i <= 43)) * (j == 2) * ((k >= 1) & (k <= 4))
    f["tracer1"][...] = speck * 2.0e-3 * rng.uniform(size=rho.shape) ** 4 * rho
    f["tracer2"][...] = np.roll(speck, 1, axis=2) * 4.0e-4 * rng.uniform(size=rho.shape) ** 4 * rho
    dm = coupler.get_data_manager_readwrite()
    names = {"uvel": "uvel", "vvel": "vvel", "wvel": "wvel"}
    names.update({"tracer%d" % t: n for t, n in enumerate(coupler.get_tracer_names())})
    for key, n in names.items():
        dm.get(n).copy_(torch.from_numpy(f[key]))


def _zero_maps(dycore):
    """the ten maps of the handle's last sub-cycle (mw_debug_zero_maps), (10, nz, ny + 18); None without maps"""
    from miniweatherml_amd import capi
    L, dims = capi.lib(), (C.c_int * 2)()
    n = L.mw_debug_zero_maps(dycore.h, None, 0, dims)
    if n <= 0:
        return None
    buf = np.zeros(n, dtype=np.uint32)
    assert L.mw_debug_zero_maps(dycore.h, buf.ctypes.data_as(C.c_void_p), n, dims) == n
    return buf.reshape(10, dims[0], dims[1])


def _seg_mask(lo, hi, nxi):
    """zr_seg_mask of csrc/mw_zero_rows.h for a periodic row: the segment bits of the cells lo .. hi"""
    L = (nxi + 25) // 26
    span = lambda a, b: ((2 << (b // L)) - (1 << (a // L))) << 4
    if hi - lo + 1 >= nxi:
        return span(0, nxi - 1)
    if lo < 0:
        return span(lo + nxi, nxi - 1) | span(0, hi)
    if hi >= nxi:
        return span(lo, nxi - 1) | span(0, hi - nxi)
    return span(lo, hi)


def _faces_stored(maps, nx):
    """-> bool (3 stages, tiles, nz + 1, ny): k_xz_state's predicate "the faces of level k of x tile t have a reader", from the maps Q1 .. Q3"""
    tiles = (nx + TILE - 1) // TILE
    out = []
    for s in (1, 2, 3):
        q = maps[s][:, 9:-9]
        nz = q.shape[0]
        lev = np.arange(nz + 1)
        words = q[np.clip(lev - 1, 0, nz - 1)] | q[np.clip(lev, 0, nz - 1)]
        out.append(np.stack([(words & np.uint32(_seg_mask(TILE * (t - 1) - 4, TILE * (t + 1) + 61, nx))) != 0 for t in range(tiles)]))
    return np.stack(out)


def _poison(dycore):
    from miniweatherml_amd import capi
    assert capi.lib().mw_debug_poison_handoff(dycore.h) == 0


_REFERENCE = {}


def _run(grid, seed, lean, steps=3, after_step=None, **opts):
    """-> (fields after every step, stored-faces predicate of the first step or None, redone stages per step, flag bytes after every step)"""
    from miniweatherml_amd import modules
    nx, ny, nz = grid
    coupler, dycore, _ = modules.make_supercell(nx, ny, nz, 1, 500.0 * nx, 500.0 * ny, 20000.0, ord=5)
    for k_, v in {"zero_verify": 1, "lean_stores": lean, **opts}.items():
        dycore.set_option(k_, v)
    if seed == "rim":
        _seed_rim(coupler)
    else:
        _seed_box(coupler, seed)
    dt = dycore.compute_time_step(coupler)
    fields, redo, flags, stored = [], [], [], None
    for n in range(steps):
        _poison(dycore)
        dycore.time_step(coupler, dt)
        redo.append(dycore.vapour_redo())
        fields.append(gpu_fields(coupler))
        flags.append(dycore.tracer_flags().reshape(nz, ny, nx))
        if n == 0:
            maps = _zero_maps(dycore)
            stored = None if maps is None else _faces_stored(maps, nx)
        if after_step is not None:
            after_step(n, coupler)
    assert dycore.path() == PATH
    nviol, kinds = dycore.zero_violations()
    assert nviol == (0 if stored is not None else -1), (nviol, kinds)
    return fields, stored, redo, flags


def _check(grid, seed, redo_expected=(0, 0, 0), after_step=None, **opts):
    new = _run(grid, seed, 1, after_step=after_step, **opts)
    key = (grid, seed, tuple(sorted(opts.items())), after_step)
    if key not in _REFERENCE:                                    # lean_stores = 0 on the same state and options: computed once and shared
        _REFERENCE[key] = _run(grid, seed, 0, after_step=after_step, **opts)
    old = _REFERENCE[key]
    what = "lean_stores %s %s %s" % (grid, seed, sorted(opts.items()))
    for n, (a, b) in enumerate(zip(new[0], old[0])):
        assert sorted(a) == sorted(b) and len(a) == 8
        for f in a:
            assert not np.isnan(b[f]).any(), (what, "lean_stores = 0", n, f)
            assert np.array_equal(a[f], b[f]), (what, "step %d" % (n + 1), f, float(np.nanmax(np.abs(a[f] - b[f]))), int(np.isnan(a[f]).sum()))
    assert new[2] == old[2] and (redo_expected is None or new[2] == list(redo_expected)), (new[2], old[2])
    for n, (a, b) in enumerate(zip(new[3], old[3])):
        assert np.array_equal(a, b), (what, "flag bytes after step %d" % (n + 1))
    record_comparison(what)
    return new


def test_option_default_and_errors(mw):
    from miniweatherml_amd import modules
    from miniweatherml_amd.capi import MWError
    coupler, dycore, _ = modules.make_supercell(24, 20, 10, 1, 12000., 10000., 20000.)
    assert dycore.get_option("lean_stores") == 1
    for v in (0, 1):
        dycore.set_option("lean_stores", v)
        assert dycore.get_option("lean_stores") == v
    for bad in (-1, 2):
        with pytest.raises(MWError):
            dycore.set_option("lean_stores", bad)


# (grid, box): lean and full levels on every grid; 70 x 40: lean and full rows too; 180 cells: lean and full x tiles (cloud in tile 0 only)
# 300 cells: tiles that leave out every face between tiles that store theirs
MIXED = [((70, 12, 20), (2, 3, 2, 3, 16, 43)), ((70, 40, 20), (2, 3, 2, 3, 16, 43)), ((180, 12, 20), (2, 3, 2, 3, 20, 26)),
         ((300, 12, 20), (2, 3, 2, 3, 20, 26))]


@pytest.mark.parametrize("chunk_z", [0, 5])
@pytest.mark.parametrize("grid,box", MIXED)
def test_mixed_lean_and_full_tiles(mw, grid, box, chunk_z):
    _, stored, _, _ = _check(grid, box, chunk_z=chunk_z)
    nx, ny, nz = grid
    assert stored is not None and stored.shape == (3, (nx + TILE - 1) // TILE, nz + 1, ny)
    for s in range(3):
        assert stored[s].any() and not stored[s].all(), s       # every stage leaves some faces out and stores some
        assert stored[s][0, 2, 2] and not stored[s][0, nz, 2]    # next to the box / at the model top
    if ny == 40:
        assert not stored[2][:, :, 20].any() and stored[2][0, 2, 11]   # stage 3 reaches nine rows: row 20 is out of reach, row 11 within
    if nx == 180:
        # four tiles, the last one partial: a tile and its two neighbours span 182 cells, the whole row -- what differs from tile to tile here is
        # the tracer kernel's form (tiles 1 and 2 are lean at every level), and every tile has to store what its neighbours' halo lanes read
        assert stored[0][:, 2, 2].all()
    if nx == 300:
        # six tiles, cloud in cells 20 .. 26 sets the segments of the cells 0 .. 35: the tiles 2 and 3 (cells 54 .. 235, 112 .. 293 with their
        # neighbours) leave out every face, the tiles 0, 1, 4 and 5 (whose span reaches the cloud, 4 and 5 round the seam) store theirs
        assert not stored[:, 2:4].any() and all(stored[0][t, 2, 2] for t in (0, 1, 4, 5))


@pytest.mark.parametrize("grid,box", [MIXED[0], MIXED[2]])
def test_forced_redo_is_replayed(mw, grid, box):
    """debug_vapour_redo: every stage's word is set by hand behind k_xz_state, the replay launch stores what the first launch left out and the
    tracer stage's three-tracer form -- which reads all of it -- redoes the vapour: same bits, three stages counted per step."""
    _, stored, redo, _ = _check(grid, box, redo_expected=(3, 3, 3), chunk_z=5, debug_vapour_redo=1)
    assert redo == [3, 3, 3] and not stored.all()


@pytest.mark.parametrize("chunk_z", [65, 70])
@pytest.mark.parametrize("levels", [(0, 1), (63, 65)])
def test_chunks_of_more_than_64_levels(mw, levels, chunk_z):
    """70 levels in chunks of 65 + 5 and of 70: the face bits of the levels from 64 on come from the second fetch.  Cloud on the levels 0 .. 1: the
    faces of the first word are stored up to level 10 or more and everything in the second word is left out; around level 64: the other way
    round, the second word's faces have readers over lean bits in the first."""
    nz = 70
    _, stored, _, _ = _check((70, 12, nz), levels + (2, 3, 16, 43), chunk_z=chunk_z)
    low = levels == (0, 1)
    for s in range(3):
        assert bool(stored[s][0, 1, 2]) == low and bool(stored[s][0, 64, 2]) == (not low) and bool(stored[s][0, 30, 2]) is False
    _check((70, 12, nz), levels + (2, 3, 16, 43), redo_expected=(3, 3, 3), chunk_z=chunk_z, debug_vapour_redo=1)


@pytest.mark.parametrize("x", [57, 58, 179, 0])
def test_box_next_to_a_tile_seam(mw, x):
    """180 cells, tiles 0 .. 57 | 58 .. 115 | 116 .. 173 | 174 .. 179.  A one-cell-wide box on the last cell of tile 0, on the first of tile 1, and
    on either side of the periodic seam: the tracer waves of the full tiles read, with their halo lanes, the edge faces of a neighbour tile whose
    own segments are clear -- that neighbour must have stored them."""
    _, stored, _, _ = _check((180, 12, 20), (2, 3, 2, 3, x, x), chunk_z=5)
    assert stored[0][:, 2, 2].all() and not stored.all()         # (every tile's span reaches the box on 180 cells; the upper levels are left out)


def test_flag_bytes_after_a_step_that_scales_nothing(mw):
    """Step 1 on the rim state: y faces are scaled, flag bytes are set.  Then cloud and rain are cleared: in steps 2 and 3 nothing is scaled,
    every tracer wave leaves early, and only the first launch behind a launch that set a byte still stores its zeros.  No byte of step 1 may be
    left after step 2 or step 3, and the bytes equal those of lean_stores = 0 after every step."""
    def clear(n, coupler):
        if n == 0:
            dm = coupler.get_data_manager_readwrite()
            for name in ("cloud_liquid", "precip_liquid"):
                dm.get(name).zero_()
    _, _, _, flags = _check((70, 12, 20), "rim", redo_expected=None, after_step=clear)
    assert np.count_nonzero(flags[0]) > 0
    assert np.count_nonzero(flags[1]) == 0 and np.count_nonzero(flags[2]) == 0
