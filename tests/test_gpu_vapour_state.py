"""Option vapour_state (default 1): in the folded supercell configuration with one member, on the one-stream schedule behind k_y_all, the water
vapour is advanced by k_xz_state next to the state variables (k_xz_state<.., VAP>) and the fused tracer stage works on cloud and rain only
(k_tracers_fused<.., VS = 1>).  A stage in which a vapour cell fails the limiter test is redone by the tracer stage's three-tracer bodies.
Results are bit for bit those of vapour_state = 0; both forms are held to the oracle at the production tolerances.

Grid 70 x 8 x 20 with chunk_z = chunk_f = 8: two x tiles (58 + 12 cells: a tile edge and a partial tile), two groups of
four rows, three z chunks with a short last one.  One CFL step and one step of twice that: the second has two sub-cycles, so the last stage
runs in its slab form and in its coupler form.

(The zero-row maps exist for blocks of at least nine rows -- a tracer must not cross a whole block within a sub-cycle -- so on eight rows every
row is full and option zero_verify has nothing to check.  The cases that are about lean rows therefore run on the common grid AND on
70 x 12 x 20, three groups of four rows, where the maps are built and their claims verified.)"""
import numpy as np
import pytest

from util import compare_fields, gpu_fields, push_fields, record_comparison

pytestmark = pytest.mark.gpu

NX, NY, NZ = 70, 8, 20
XLEN, YLEN, ZLEN = 500.0 * NX, 500.0 * NY, 20000.0
ORDERS = [5]                                                    # (the vapour form exists for WENO-5; WENO-3 keeps the tracer stage)
CHUNKS = {"chunk_z": 8, "chunk_f": 8}


NY_MAPS = 12                                                    # rows of the second grid: the smallest multiple of four on which the maps exist


def _blob_mask(ny=NY):
    """bench.py's developed-state pattern -- smooth blobs with sharp rims -- scaled to this grid."""
    i = np.arange(NX, dtype=np.float64).reshape(1, 1, NX, 1)
    j = np.arange(ny, dtype=np.float64).reshape(1, ny, 1, 1)
    return ((np.sin(i * 0.11 * 400.0 / NX) * np.cos(j * 0.07 * 400.0 / NY)) > 0.3).astype(np.float64)


def _seed(f, state):
    """f: dict of numpy fields (oracle naming), changed in place.  clear: the cloud-free initial state.  blobs: cloud and rain blobs with sharp
    rims confined to rows 2 .. 3, cells 16 .. 43 and the lowest levels, so that lean and full x tiles, rows and levels mix in every stage (the
    second x tile, row 6 in stage 1 and the upper levels stay lean).  rim: single cloud / rain cells of very different size side by side in one
    row, in a strong random wind: their multipliers drop below 1 and y faces are scaled next to rows that are lean in the next step's first
    stage.  masked: the vapour times the blob mask -- exact zeros next to non-zero cells in the sheared wind."""
    rho = f["density_dry"]
    ny = rho.shape[1]
    k = np.arange(NZ, dtype=np.float64).reshape(NZ, 1, 1, 1)
    i = np.arange(NX, dtype=np.float64).reshape(1, 1, NX, 1)
    j = np.arange(ny, dtype=np.float64).reshape(1, ny, 1, 1)
    if state == "blobs":
        box = _blob_mask(ny) * ((i >= 16) & (i <= 43)) * ((j >= 2) & (j <= 3))
        f["tracer1"][...] = 2.0e-3 * box * ((k >= 2) & (k <= 3)) * (0.5 + 0.5 * np.sin(0.3 * k + 0.05 * i) ** 2) * rho
        f["tracer2"][...] = 4.0e-4 * box * (k <= 2) * (0.5 + 0.5 * np.cos(0.2 * k + 0.03 * j) ** 2) * rho
    elif state == "rim":
        rng = np.random.default_rng(7)
        for n, amp in (("uvel", 25.0), ("vvel", 25.0), ("wvel", 8.0)):
            f[n] += amp * rng.uniform(-1, 1, f[n].shape)
        speck = (rng.uniform(size=rho.shape) > 0.5) * ((i >= 16) & (i <= 43)) * (j == 2) * ((k >= 1) & (k <= 4))
        f["tracer1"][...] = speck * 2.0e-3 * rng.uniform(size=rho.shape) ** 4 * rho
        f["tracer2"][...] = np.roll(speck, 1, axis=2) * 4.0e-4 * rng.uniform(size=rho.shape) ** 4 * rho
    elif state == "masked":
        f["tracer0"] *= _blob_mask(ny)
    else:
        assert state == "clear"


def _gpu_case(modules, order, state, ny=NY, **opts):
    coupler, dycore, _ = modules.make_supercell(NX, ny, NZ, 1, XLEN, 500.0 * ny, ZLEN, ord=order)
    for k_, v in {**CHUNKS, **opts}.items():
        dycore.set_option(k_, v)
    f = gpu_fields(coupler)
    _seed(f, state)
    import torch
    dm = coupler.get_data_manager_readwrite()
    names = {"density_dry": "density_dry", "uvel": "uvel", "vvel": "vvel", "wvel": "wvel", "temp": "temp"}
    names.update({"tracer%d" % t: n for t, n in enumerate(coupler.get_tracer_names())})
    for key, n in names.items():
        dm.get(n).copy_(torch.from_numpy(f[key]))
    return coupler, dycore


def _run(modules, order, state, factors=(1.0, 2.0), ny=NY, **opts):
    """-> (fields after the steps, redo stages per step)"""
    coupler, dycore = _gpu_case(modules, order, state, ny=ny, **opts)
    dt = dycore.compute_time_step(coupler)
    redo = []
    for fac in factors:
        dycore.time_step(coupler, dt * fac)
        redo.append(dycore.vapour_redo())
    out = gpu_fields(coupler)
    if opts.get("zero_verify"):
        nviol, kinds = dycore.zero_violations()
        assert nviol == (0 if (ny >= 9 and opts.get("zero_rows", 1)) else -1), (nviol, kinds, order, state, ny, opts)   # (-1: no maps, the check never ran)
    assert dycore.path() == "march ord%d K1 nens1 one_stream y_all conv_in_y tracers_fused 3d" % order
    return out, redo


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b) and len(a) == 8
    for k_ in a:
        assert np.array_equal(a[k_], b[k_]), (what, k_, float(np.max(np.abs(a[k_] - b[k_]))))
    record_comparison(what)


def test_option_defaults_and_errors(mw):
    from miniweatherml_amd import modules
    from miniweatherml_amd.capi import MWError
    coupler, dycore, _ = modules.make_supercell(24, 20, 10, 1, 12000., 10000., 20000.)
    assert dycore.get_option("vapour_state") == 1 and dycore.get_option("debug_vapour_redo") == 0
    assert dycore.vapour_redo() == 0                             # (no time step yet)
    for key in ("vapour_state", "debug_vapour_redo"):
        for v in (0, 1):
            dycore.set_option(key, v)
            assert dycore.get_option(key) == v
        for bad in (-1, 2):
            with pytest.raises(MWError):
                dycore.set_option(key, bad)


@pytest.mark.parametrize("order", ORDERS)
def test_cloud_free_same_bits_no_redo(mw, order):
    from miniweatherml_amd import modules
    new, redo = _run(modules, order, "clear")
    old, redo0 = _run(modules, order, "clear", vapour_state=0)
    _assert_same_bits(new, old, "vapour_state cloud-free ord%d" % order)
    assert redo == [0, 0] and redo0 == [0, 0]


@pytest.mark.parametrize("ny", [NY, NY_MAPS])
@pytest.mark.parametrize("maps", [1, 0])
@pytest.mark.parametrize("order", ORDERS)
def test_cloud_and_rain_blobs_same_bits(mw, order, maps, ny):
    """(2a / 2b) lean and full tiles, rows and levels mixed, with the maps' claims verified; and without maps: every row full."""
    from miniweatherml_amd import modules
    new, redo = _run(modules, order, "blobs", ny=ny, zero_rows=maps, zero_verify=1)
    old, _ = _run(modules, order, "blobs", ny=ny, zero_rows=maps, zero_verify=1, vapour_state=0)
    _assert_same_bits(new, old, "vapour_state blobs ord%d maps %d ny %d" % (order, maps, ny))
    assert redo == [0, 0]
    assert float(np.max(new["tracer1"])) > 0 and float((new["tracer1"] == 0).mean()) > 0.3


@pytest.mark.parametrize("ny", [NY, NY_MAPS])
@pytest.mark.parametrize("order", ORDERS)
def test_flag_bytes_next_to_lean_rows(mw, order, ny):
    """(2c) Cloud cells whose multiplier drops below 1 scale y faces (flag bytes set, the correction pass at work) in a row whose neighbours are
    lean in the next step's first stage.  k_tracer_patch scans the neighbouring rows' bytes, so waves that leave early store zero bytes.
    What this shows: three steps with the same bits on a state where the correction pass has work to do (without it the result differs),
    with lean rows beside flagged ones on the twelve-row grid (on eight rows there are no maps and no wave leaves early).  What it does
    NOT show: that a stale byte was really met -- nothing reads the flag array back, and there is no switch that leaves the zero-byte
    stores out."""
    from miniweatherml_amd import modules
    f3 = (1.0, 1.0, 1.0)
    new, redo = _run(modules, order, "rim", factors=f3, ny=ny, zero_verify=1)
    assert redo == [0, 0, 0], redo                               # (the vapour itself is smooth: the form without it is what runs here)
    old, _ = _run(modules, order, "rim", factors=f3, ny=ny, vapour_state=0)
    _assert_same_bits(new, old, "vapour_state rim ord%d ny %d" % (order, ny))
    nopatch, _ = _run(modules, order, "rim", factors=f3, ny=ny, vapour_state=0, debug_no_patch=1)
    assert any(not np.array_equal(nopatch[k_], old[k_]) for k_ in ("tracer1", "tracer2"))


def test_early_leaving_waves_clear_stale_flag_bytes(mw):
    """(2c, the hazard itself.)  By construction of the maps a row cannot be lean right after a stage in which it was flagged as long as the
    dycore alone moves the tracers: the non-zero set only grows.  It shrinks when something else clears cloud and rain between two steps
    (Kessler's evaporation does).  So: 70 x 40 x 20; step 1 on the rim state around row 2, whose limiter sets flag bytes there (read back:
    non-zero bytes exist); then cloud and rain are cleared and the same specks are seeded in rows 20 .. 24; step 2.  Rows 34 .. 39 and 0 .. 10 are lean in
    every stage of step 2, their waves leave early, while y faces are scaled around row 22, so k_tracer_patch scans bytes.  The bytes of
    the rows that were flagged in step 1 must be zero afterwards -- they are only if the leaving waves stored them -- and the fields
    equal those of vapour_state = 0 bit for bit."""
    import torch
    from miniweatherml_amd import modules
    ny, res = 40, []
    for vap in (1, 0):
        coupler, dycore = _gpu_case(modules, 5, "rim", ny=ny, vapour_state=vap, zero_verify=1)
        dt = dycore.compute_time_step(coupler)
        dycore.time_step(coupler, dt)
        fl1 = dycore.tracer_flags().reshape(NZ, ny, NX)
        rows1 = sorted(set(np.nonzero(fl1)[1].tolist()))
        assert rows1 and set(rows1) <= set(range(0, 9)) | set(range(34, ny)), rows1   # flagged cells around row 2 (periodic), within the reach of one step
        dm = coupler.get_data_manager_readwrite()
        for n in ("cloud_liquid", "precip_liquid"):
            t = dm.get(n)
            moved = torch.roll(torch.where(t > 1e-7, t, torch.zeros_like(t)), 20, dims=1)   # the specks themselves (not the step's tiny spread), 20 rows on
            moved[:, :20] = 0.0; moved[:, 25:] = 0.0               # rows 20 .. 24: the last stage's full rows are 11 .. 33
            t.copy_(moved)
        dycore.time_step(coupler, dt)
        assert dycore.vapour_redo() == 0
        fl2 = dycore.tracer_flags().reshape(NZ, ny, NX)
        assert np.count_nonzero(fl2[:, 11:34]) > 0                # y faces were scaled in step 2: the correction pass scanned flag bytes
        lean2 = np.concatenate([fl2[:, :11], fl2[:, 34:]], axis=1)   # the rows that were lean in every stage of step 2 hold all of step 1's flags
        assert np.count_nonzero(lean2) == 0, np.argwhere(lean2)[:5]
        nviol, kinds = dycore.zero_violations()
        assert nviol == 0, kinds
        res.append(gpu_fields(coupler))
    _assert_same_bits(res[0], res[1], "vapour_state stale flag bytes")


@pytest.mark.parametrize("order", ORDERS)
def test_vapour_limiter_acts_redo_same_bits(mw, oracle, order):
    """(3) Exact zeros next to non-zero vapour in the sheared wind: cells fail the limiter test, the stages are redone, same bits.  That the
    seeded state really makes the limiter scale a vapour flux is checked on the CPU oracle: without the vapour's limiter it ends up elsewhere."""
    from miniweatherml_amd import modules
    new, redo = _run(modules, order, "masked")
    old, redo0 = _run(modules, order, "masked", vapour_state=0)
    print("redo stages per step:", redo)
    assert redo[0] > 0 and redo[1] > 0 and redo0 == [0, 0]
    _assert_same_bits(new, old, "vapour_state masked vapour ord%d" % order)
    O = oracle.with_order(order) if order != 5 else oracle
    ends = []
    for positive in ((1, 1, 1), (0, 1, 1)):
        p, _ = O.make_params(NX, NY, NZ, 1, XLEN, YLEN, ZLEN)
        odyc = O.OracleDycore(p, tracer_positive=list(positive), tracer_adds_mass=[1, 1, 1])
        of = O.Fields(odyc.p)
        odyc.init("supercell", of)
        of.tracers[0] *= _blob_mask()
        odyc.time_step(of, odyc.compute_time_step())
        ends.append(of.tracers[0].copy())
    assert np.max(np.abs(ends[0] - ends[1])) > 1e-9 * np.max(np.abs(ends[0]))


@pytest.mark.parametrize("state", ["clear", "blobs"])
@pytest.mark.parametrize("order", ORDERS)
def test_forced_redo_same_bits(mw, order, state):
    """(4) debug_vapour_redo: every stage's word set by hand, the tracer stage overwrites a vapour that needed no redo with the same bits."""
    from miniweatherml_amd import modules
    new, redo = _run(modules, order, state, debug_vapour_redo=1)
    old, _ = _run(modules, order, state, vapour_state=0)
    assert redo == [3, 6], redo                                  # (three stages per sub-cycle; the second step has two sub-cycles)
    _assert_same_bits(new, old, "vapour_state forced redo %s ord%d" % (state, order))


@pytest.mark.parametrize("vap", [1, 0])
@pytest.mark.parametrize("state", ["clear", "blobs"])
@pytest.mark.parametrize("order", ORDERS)
def test_against_the_oracle(mw, oracle, order, state, vap):
    """(5) Production tolerances: 1e-11 after one step, 1e-9 after ten; the default form and vapour_state = 0 (the three-tracer instantiations
    stay compiled: this is where they meet the oracle), both states, both orders.  The second step is sub-cycled."""
    from miniweatherml_amd import modules
    O = oracle.with_order(order) if order != 5 else oracle
    coupler, dycore, _ = modules.make_supercell(NX, NY, NZ, 1, XLEN, YLEN, ZLEN, ord=order)
    for k_, v in {**CHUNKS, "vapour_state": vap}.items():
        dycore.set_option(k_, v)
    odyc, of = O.supercell_setup(NX, NY, NZ, 1, XLEN, YLEN, ZLEN)
    f = of.as_dict()
    _seed(f, state)
    for t in range(3):
        of.tracers[t][...] = f["tracer%d" % t]
    push_fields(coupler, of)
    dt = dycore.compute_time_step(coupler)
    what = "vapour_state=%d %s ord%d" % (vap, state, order)
    for step in range(10):
        fac = 2.0 if step == 1 else 1.0
        dycore.time_step(coupler, dt * fac)
        odyc.time_step(of, dt * fac)
        if step == 0:
            compare_fields(gpu_fields(coupler), of.as_dict(), 1e-11, what + ", 1 step")
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-9, what + ", 10 steps")
    assert dycore.vapour_redo() == 0
