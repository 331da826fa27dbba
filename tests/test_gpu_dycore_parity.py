"""GPU parity of Dynamics_Euler_Stratified_WenoFV (C ABI -> HIP kernels) against the CPU oracle on identical inputs.

Tolerances (derived from the reference's own FMA-contraction sensitivity):
    per field  max|diff| <= 1e-11 * max|field| after 1 dycore step,  <= 1e-9 * max|field| after 10 steps.
Kernel paths:  0 production (marching kernels, re-associated arithmetic), 1 strict (reference operation order,
contraction off), 2 general kernels with the fast arithmetic."""
import json
import os

import numpy as np
import torch
import pytest

from util import compare_fields, record_comparison, gpu_fields, oracle_sensitivity, push_fields, sens_allowed, set_options

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SNAP = json.load(open(os.path.join(HERE, "golden", "oracle_snapshots.json")))
KA = json.load(open(os.path.join(HERE, "golden", "baseline_known_answers.json")))


def setup_case(oracle, case, nranks=1, rank=0):
    from miniweatherml_amd import modules
    nx, ny, nz, nens, xlen, ylen, zlen, init, nt, grav, nsteps = case
    micro = None
    if nt == 1:                                           # simple_city driver: only water_vapor is registered (driver.cpp:55-56)
        class OneTracer(modules.Microphysics_Kessler):
            def init(self, coupler):
                coupler.add_tracer("water_vapor", "Water Vapor", True, True)
        micro = OneTracer()
    coupler, dycore, _ = modules.make_supercell(nx, ny, nz, nens, xlen, ylen, zlen, init, micro=micro, enable_gravity=grav,
                                                perturb=(init == "supercell"))
    odyc, of = oracle.supercell_setup(nx, ny, nz, nens, xlen, ylen, zlen, init_data=init, num_tracers=nt, enable_gravity=grav,
                                      perturb=(init == "supercell"))
    return coupler, dycore, odyc, of


def case_sensitivity(oracle, name, steps):
    nx, ny, nz, nens, xlen, ylen, zlen, init, nt, grav, nsteps = SNAP["cases"][name]
    make = lambda: oracle.supercell_setup(nx, ny, nz, nens, xlen, ylen, zlen, init_data=init, num_tracers=nt,   # noqa: E731
                                          enable_gravity=grav, perturb=(init == "supercell"))
    return oracle_sensitivity(oracle, name, make, steps)


@pytest.mark.parametrize("name", sorted(SNAP["cases"]))
def test_init_matches_oracle(mw, oracle, name):
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"][name])
    hy = odyc.hy()
    for k in ("hy_dens_cells", "hy_dens_theta_cells", "hy_dens_edges", "hy_dens_theta_edges"):
        assert np.array_equal(getattr(dycore, k), hy[k]), k          # host column code, same libm -> bitwise
    # init + perturb_temperature: the device code keeps the reference's operation order, and its pow, exp and cos have glibc's bits
    # (csrc/mw_glibc_pow.h): BIT-identical to the oracle, all four initial states
    compare_fields(gpu_fields(coupler), of.as_dict(), 0.0, "init %s, strict arithmetic: mode 1" % name)
    assert np.array_equal(dycore.immersed_proportion(coupler).cpu().numpy(), odyc.immersed_proportion())
    assert coupler.get_option("use_immersed_boundaries") == bool(odyc.p.use_immersed)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(SNAP["cases"]))
def test_time_steps_match_oracle(mw, oracle, name, mode):
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"][name])
    push_fields(coupler, of)                                          # identical inputs on both sides
    dycore.set_strict(mode)
    dt = dycore.compute_time_step(coupler)
    assert dt == odyc.compute_time_step()
    # the sensitivity fallback only for the allow-listed thermal case (tests/util.py: SENS_ALLOW); plain 1e-11 / 1e-9 elsewhere
    sens = case_sensitivity(oracle, name, (1, 10)) if sens_allowed(name) else {1: None, 10: None}
    dycore.time_step(coupler, dt)
    odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-11, "%s mode %d, 1 step" % (name, mode), sens[1])
    for _ in range(9):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-9, "%s mode %d, 10 steps" % (name, mode), sens[10])
    assert abs(dycore.etime - 10 * dt) < 1e-12


@pytest.mark.parametrize("mode", [1, 2])
def test_compute_tendencies_and_fluxes(mw, oracle, mode):
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"]["supercell3d_16x16x8"])
    push_fields(coupler, of)
    dycore.set_strict(mode)
    dt = dycore.compute_time_step(coupler)
    st, tt = dycore.compute_tendencies(coupler, dt)
    ost, ott = odyc.stage_tendencies(of, dt)
    check_fluxes(dycore, coupler, odyc, 1e-13 if mode == 1 else 1e-11)
    tol = 1e-11 if mode == 1 else 1e-9
    for got, ref in ((st.cpu().numpy(), ost), (tt.cpu().numpy(), ott)):
        for v in range(ref.shape[0]):
            assert np.max(np.abs(got[v] - ref[v])) <= tol * max(np.max(np.abs(ref[v])), 1e-300)


def check_fluxes(dycore, coupler, odyc, tol):
    ofl = odyc.fluxes()
    gfl = {k: v.cpu().numpy() for k, v in dycore.fluxes(coupler).items()}
    # scale per variable = largest flux of that variable over the three directions (a y-flux that is a pure cancellation
    # residue of the symmetric set-up must not be judged against its own tiny magnitude)
    for grp in ("state_flux_", "tracers_flux_"):
        for v in range(ofl[grp + "x"].shape[0]):
            scale = max(np.max(np.abs(ofl[grp + d][v])) for d in "xyz")
            for d in "xyz":
                assert gfl[grp + d].shape == ofl[grp + d].shape
                err = np.max(np.abs(gfl[grp + d][v] - ofl[grp + d][v]))
                assert err <= tol * scale + 1e-300, (grp + d, v, err, scale)
    record_comparison("six public flux arrays against the oracle's, tol %g of each variable's largest flux" % tol)


@pytest.mark.parametrize("mode", [0, 1])
def test_public_flux_arrays_after_time_step(mw, oracle, mode):
    """state_flux_* / tracers_flux_* are registered 'so the user has access' (:1671-1676): after time_step they hold the
    last RK stage's post-FCT fluxes.  The production path rebuilds the state part on demand."""
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"]["supercell3d_16x16x8"])
    push_fields(coupler, of)
    dycore.set_strict(mode)
    dt = dycore.compute_time_step(coupler)
    for _ in range(2):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    check_fluxes(dycore, coupler, odyc, 1e-10)


def test_subcycling_dt_phys_larger_than_cfl(mw, oracle):
    """dt_phys > dt_dyn -> ncycles = ceil(dt_phys/dt_dyn) sub-cycles (:104-110)."""
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"]["supercell3d_16x16x8"])
    push_fields(coupler, of)
    dt = 2.5 * dycore.compute_time_step(coupler)
    dycore.time_step(coupler, dt)
    odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-10, "3 sub-cycles")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bc", [(2, 0, 2), (1, 0, 2), (0, 2, 2), (2, 2, 2), (1, 1, 1)])
def test_wall_and_open_boundaries(mw, oracle, mode, bc):
    """bc_x / bc_y wall (2) and open (1), incl. the reference's single-rank `else if` quirk."""
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"]["thermal3d_16x16x16"])
    push_fields(coupler, of)
    dycore.set_strict(mode)
    dycore.set_bc(coupler, *bc)
    odyc.p.bc_x, odyc.p.bc_y, odyc.p.bc_z = bc
    dt = dycore.compute_time_step(coupler)
    for _ in range(3):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    sens = case_sensitivity(oracle, "thermal3d_16x16x16", (3,))      # periodic-BC sensitivity as the yardstick
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-10, "bc %s mode %d" % (bc, mode), sens[3])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("bc", [(0, 0, 0), (2, 1, 0)])
def test_z_periodic(mw, oracle, mode, bc):
    """bc_z = periodic (halo rule :752-763, edge rule :1008-1019: the boundary faces take the finished edge values of the opposite
    boundary face, hydrostatic part of that level included).  No shipped case uses it; the thermal bubble case with its z-periodic
    rule switched on is the test (1e-11 after 1 step, 1e-9 after 10; the thermal case is on the sensitivity allow-list)."""
    coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"]["thermal3d_16x16x16"])
    push_fields(coupler, of)
    dycore.set_strict(mode)
    dycore.set_bc(coupler, *bc)
    odyc.p.bc_x, odyc.p.bc_y, odyc.p.bc_z = bc
    dt = dycore.compute_time_step(coupler)
    sens = case_sensitivity(oracle, "thermal3d_16x16x16", (1, 10))
    dycore.time_step(coupler, dt)
    odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-11, "zperiodic %s mode %d, 1 step" % (bc, mode), sens[1])
    check_fluxes(dycore, coupler, odyc, 1e-9)                 # incl. the two boundary faces, which must carry the same flux
    fz = dycore.fluxes(coupler)["state_flux_z"]
    assert float((fz[:, 0] - fz[:, -1]).abs().max()) == 0.0
    for _ in range(9):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-9, "zperiodic %s mode %d, 10 steps" % (bc, mode), sens[10])


def test_z_periodic_differs_from_wall(mw, oracle):
    """Negative control: the periodic z rule is really applied (the same run with the wall rule gives a different state)."""
    out = []
    for bcz in (0, 2):
        coupler, dycore, odyc, of = setup_case(oracle, SNAP["cases"]["thermal3d_16x16x16"])
        push_fields(coupler, of)
        dycore.set_bc(coupler, 0, 0, bcz)
        dt = dycore.compute_time_step(coupler)
        for _ in range(3):
            dycore.time_step(coupler, dt)
        out.append(gpu_fields(coupler))
    assert np.max(np.abs(out[0]["wvel"] - out[1]["wvel"])) > 1e-6


def test_known_answers_on_gpu(mw, oracle):
    """32x32x16 supercell + bubble, 3 dycore steps (reference-run numbers)."""
    from miniweatherml_amd import modules
    ref = KA["supercell_32x32x16_3steps"]
    coupler, dycore, micro = modules.make_supercell(32, 32, 16, 1, 16000., 16000., 20000.)
    dt = dycore.compute_time_step(coupler)
    assert dt == KA["dt_32x32x16"]
    g = gpu_fields(coupler)
    assert abs(g["density_dry"].sum() - ref["density_dry_sum_init"]) <= 1e-12 * ref["density_dry_sum_init"]
    for _ in range(3):
        dycore.time_step(coupler, dt)
    g = gpu_fields(coupler)
    assert abs(g["wvel"].max() - ref["wvel_max"]) <= 1e-10
    assert abs(g["wvel"].min() - ref["wvel_min"]) <= 1e-10
    assert abs(g["temp"].max() - ref["temp_max"]) <= 1e-10 * ref["temp_max"]
    assert abs(g["density_dry"].sum() - ref["density_dry_sum_after"]) <= 1e-11 * ref["density_dry_sum_after"]


def test_many_tracers_general_grouping(mw, oracle):
    """7 tracers: the tracer kernels run in groups of <= 4."""
    from miniweatherml_amd import modules

    class ManyTracers(modules.Microphysics_Kessler):
        def init(self, coupler):
            super().init(coupler)
            for n in range(4):
                coupler.add_tracer("extra%d" % n, "passive", n % 2 == 0, False)

    coupler, dycore, _ = modules.make_supercell(12, 12, 8, 1, 6000., 6000., 20000., micro=ManyTracers())
    p, _ = oracle.make_params(12, 12, 8, 1, 6000., 6000., 20000., num_tracers=7)
    odyc = oracle.OracleDycore(p, tracer_positive=[1, 1, 1, 1, 0, 1, 0], tracer_adds_mass=[1, 1, 1, 0, 0, 0, 0])
    of = oracle.Fields(odyc.p)
    odyc.init("supercell", of)
    oracle.perturb_temperature(odyc.p, of.temp)
    rng = np.random.default_rng(5)
    for t in range(3, 7):
        of.tracers[t][...] = rng.uniform(0.0, 1e-3, of.tracers[t].shape) * (1 if t % 2 else (rng.uniform(size=of.tracers[t].shape) > 0.5))
    push_fields(coupler, of)
    dt = dycore.compute_time_step(coupler)
    for _ in range(3):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-10, "7 tracers")


RAGGED = {
    # name: (nx, ny, nz, nens, xlen, ylen, zlen, init_data, num_tracers, enable_gravity, nsteps)
    "ragged_37x11x5_nens3": (37, 11, 5, 3, 18500., 5500., 20000., "supercell", 3, True, 2),       # x tiles of 58 fused lanes (19 cells), nens 3
    "ragged_130x7x9": (130, 7, 9, 1, 65000., 3500., 20000., "supercell", 3, True, 2),             # 3 x tiles, 2 z chunks
    "ragged2d_70x1x6": (70, 1, 6, 1, 35000., 1.0e5, 20000., "supercell", 3, True, 2),             # 2-D, 2 x tiles
    "ragged_3x3x3": (3, 3, 3, 1, 1500., 1500., 20000., "supercell", 3, True, 2),                  # the smallest legal grid
    "ragged_50x6x7_nens4": (50, 6, 7, 4, 25000., 3000., 20000., "supercell", 3, True, 2),          # nens 4: 4 x tiles (state), 5 (fused)
    "ragged_9x4x6_nens12": (9, 4, 6, 12, 4500., 2000., 20000., "supercell", 3, True, 1),           # the widest ensemble the fused stage takes
    "ragged_9x4x6_nens13": (9, 4, 6, 13, 4500., 2000., 20000., "supercell", 3, True, 1),           # -> unfused tracer kernels
    "ragged_20x5x33_nens10": (20, 5, 33, 10, 10000., 2500., 20000., "supercell", 3, True, 1),     # nens 10: 44 cells per wave (state), 24 (fused tracers)
}


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_sizes(mw, oracle, name, mode):
    """Tile / chunk / halo edge cases of the marching kernels (partial x tiles, several z and y chunks, nens > 1, tiny grids)."""
    case = RAGGED[name]
    coupler, dycore, odyc, of = setup_case(oracle, case)
    push_fields(coupler, of)
    dycore.set_strict(mode)
    dt = dycore.compute_time_step(coupler)
    nx, ny, nz, nens, xlen, ylen, zlen, init, nt, grav, nsteps = case
    for _ in range(nsteps):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-10, "%s mode %d" % (name, mode))


def test_unsupported_options_fail_loudly(mw):
    from miniweatherml_amd import modules
    from miniweatherml_amd.capi import MWError
    coupler, dycore, _ = modules.make_supercell(8, 8, 8, 1, 4000., 4000., 20000.)
    with pytest.raises(MWError, match="bc_x / bc_y / bc_z"):
        dycore.set_bc(coupler, 0, 0, 3)                       # not a boundary type
    with pytest.raises(MWError, match="dt_phys"):
        dycore.time_step(coupler, 0.0)


def test_a_block_whose_strides_leave_32_bits_is_refused(mw):
    """The kernels' row / level / variable strides are 32-bit values (Stride32, csrc/mw_common.h): a block with a variable of 2^31 or more
    elements (16 GB; four slabs of six of them would not fit the GPU) must be refused at create -- before any large allocation -- not
    wrapped around.  The order change that widens the halo is held to the same rule."""
    import ctypes as C
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd.capi import MWError
    L = capi.lib()
    coupler, dycore, _ = modules.make_supercell(8, 8, 8, 1, 4000., 4000., 20000.)
    g = capi.Grid()
    capi.check(L.mw_dycore_get_grid(dycore.h, C.byref(g)))
    g.nz, g.ny, g.ny_glob, g.nx, g.nx_glob = 1500, 1500, 1500, 1000, 1000        # (1504 x 1506 x 1006 = 2.28e9 elements per slab variable)
    h = C.c_void_p()
    free0 = torch_free()
    rc = L.mw_dycore_create(C.byref(h), C.byref(g), bytes([1, 1, 1]), bytes([1, 1, 1]), None)
    assert rc != 0 and "2^31" in L.mw_last_error().decode()
    assert free0 - torch_free() < (1 << 30)                                      # nothing of the 18 GB slabs was allocated on the way
    g.nz, g.ny, g.ny_glob, g.nx, g.nx_glob = 1319, 1276, 1276, 1270, 1270        # 1323 x 1282 x 1276 = 2.164e9 > 2^31 - 1 > 1319 x 1276 x 1270 ... just over
    assert L.mw_dycore_create(C.byref(h), C.byref(g), bytes([1, 1, 1]), bytes([1, 1, 1]), None) != 0


def torch_free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("overlap", ["0", "1"])
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("shape", [(70, 9, 12, 1), (23, 6, 11, 2), (64, 1, 9, 1), (64, 7, 10, 1), (20, 5, 9, 2)])
def test_fct_limiter_heavy(mw, oracle, fused, shape, monkeypatch, overlap):
    """(overlap: the two-stream schedule -- state | tracer pipelines, the default with a neighbour exchange -- or one stream.)
    Sparse cloud/rain blobs in a strong random wind: the FCT multiplier is < 1 in a large share of the cells, in all three
    directions and across wave (x tile), row and z-chunk edges.  fused=1: k_tracers_fused + k_tracer_patch (y faces scaled
    by a donor in another row are corrected afterwards); fused=0: k_xz_tracers + k_tracer_update.
    (Rows of 64 and 2 x 20 = 40 cells: k_tracer_patch reads its flag bytes as 8-byte words; 70 and 46: byte by byte.)"""
    from miniweatherml_amd import modules
    nx, ny, nz, nens = shape
    set_options(monkeypatch, fused_tracers=fused, overlap=overlap, chunk_f=4, chunk_z=4)
    xlen, ylen = 500.0 * nx, 500.0 * max(ny, 2)
    coupler, dycore, _ = modules.make_supercell(nx, ny, nz, nens, xlen, ylen, 20000.)

    def make(positive=(1, 1, 1)):
        p, _ = oracle.make_params(nx, ny, nz, nens, xlen, ylen, 20000.)
        odyc = oracle.OracleDycore(p, tracer_positive=list(positive), tracer_adds_mass=[1, 1, 1])
        of = oracle.Fields(odyc.p)
        odyc.init("supercell", of)
        rng = np.random.default_rng(11)
        for a, amp in ((of.uvel, 25.0), (of.vvel, 25.0 if ny > 1 else 0.0), (of.wvel, 8.0)):
            a += amp * rng.uniform(-1, 1, a.shape)
        for t in (1, 2):
            blob = rng.uniform(size=of.tracers[t].shape)
            of.tracers[t][...] = np.where(blob > 0.7, 2e-3 * rng.uniform(size=blob.shape), 0.0)
        return odyc, of

    odyc, of = make()
    push_fields(coupler, of)
    dt = dycore.compute_time_step(coupler)
    onof, fnof = make(positive=(1, 0, 0))                      # the same run without the limiter on cloud/rain
    for step in range(3):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
        onof.time_step(fnof, dt)
        got = gpu_fields(coupler)
        compare_fields(got, of.as_dict(), 1e-10, "limiter-heavy fused=%s step %d" % (fused, step + 1))
        assert got["tracer1"].min() >= 0 and got["tracer2"].min() >= 0
    # the limiter really was at work: without it the oracle ends up somewhere else
    assert np.max(np.abs(fnof.tracers[1] - of.tracers[1])) > 1e-3 * np.max(np.abs(of.tracers[1]))


@pytest.mark.parametrize("shape", [(70, 9, 12, 1), (64, 7, 10, 1)])
def test_fct_patch_pass_is_exercised(mw, oracle, monkeypatch, shape):
    """Negative control for the test above: with the y-face correction pass switched off the fused path must MISS the
    oracle on the limiter-heavy case (i.e. donors in neighbouring rows really do scale y faces there) -- on a row length that
    k_tracer_patch scans byte by byte and on one it scans in 8-byte words."""
    set_options(monkeypatch, debug_no_patch=1)
    with pytest.raises(AssertionError):
        test_fct_limiter_heavy(mw, oracle, "1", shape, monkeypatch, "0")


def test_large_perturbation_takes_the_pow_fallback(mw, oracle):
    """(rho theta)' beyond 5 % of the hydrostatic value: the Riemann solver's pressure series hands over to the out-of-line
    device pow (pressure_pow) on those lanes; a +-12 % temperature field exercises it on roughly half of the faces."""
    from miniweatherml_amd import modules
    coupler, dycore, _ = modules.make_supercell(20, 14, 10, 1, 10000., 7000., 20000.)
    odyc, of = oracle.supercell_setup(20, 14, 10, 1, 10000., 7000., 20000.)
    rng = np.random.default_rng(21)
    of.temp *= 1.0 + rng.uniform(-0.12, 0.12, of.temp.shape)
    push_fields(coupler, of)
    dt = 0.25 * dycore.compute_time_step(coupler)              # a violent state: small steps
    for step in range(2):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
        compare_fields(gpu_fields(coupler), of.as_dict(), 1e-10, "large perturbation step %d" % (step + 1))


def test_non_default_gamma_uses_the_generic_pressure(mw, oracle):
    """cp_d set by the caller (options are only defaulted when absent, :1227-1249): gamma != 1003/716, so the literal series
    table does not apply and every pressure goes through the generic pow."""
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    nx, ny, nz = 16, 12, 10
    coupler = Coupler("cuda:0")
    coupler.set_option("out_prefix", "test"); coupler.set_option("init_data", "supercell"); coupler.set_option("out_freq", -1.0)
    coupler.distribute_mpi_and_allocate_coupled_state(nz, ny, nx, 1)
    coupler.set_grid(8000., 6000., 20000.)
    micro, dycore = modules.Microphysics_Kessler(), modules.Dynamics_Euler_Stratified_WenoFV()
    micro.init(coupler)
    coupler.set_option("cp_d", 1010.0)                             # after micro.init (which sets 1003), before dycore.init
    for k in ("cv_d", "gamma_d", "kappa_d", "C0"):
        if coupler.option_exists(k):
            coupler.delete_option(k)
    dycore.init(coupler)
    p, _ = oracle.make_params(nx, ny, nz, 1, 8000., 6000., 20000.)
    p.cp_d = 1010.0
    p.gamma_d = p.cp_d / (p.cp_d - p.R_d)
    p.kappa_d = p.R_d / p.cp_d
    p.C0 = oracle.lib().mwo_compute_C0(p.R_d, p.p0, p.kappa_d, p.gamma_d)
    assert coupler.grid.gamma_d == p.gamma_d and coupler.grid.C0 == p.C0
    odyc = oracle.OracleDycore(p)
    of = oracle.Fields(odyc.p)
    odyc.init("supercell", of)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-13, "init, cp_d = 1010")
    oracle.perturb_temperature(odyc.p, of.temp)
    push_fields(coupler, of)
    dt = dycore.compute_time_step(coupler)
    for step in range(2):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
        compare_fields(gpu_fields(coupler), of.as_dict(), 1e-11 if step == 0 else 1e-10, "cp_d = 1010, step %d" % (step + 1))


# ---------------------------------------------------------------------------------------------------------------------
# WENO order 3: the reference's -DMW_ORD=3 build (the only order its GPU benchmark environment compiles,
# build/machines/aws/aws_a100_gpu.env:21).  Oracle = the same restatement compiled with -DMW_ORD=3 (WenoLimiter<3>, hs = 1,
# 3-point GLL initial data); device = mw_dycore_set_order(h, 3) -> the marching kernels' ORD = 3 forms (production) or the general
# kernels with weno3_edges_* (strict / mode 2).
# ---------------------------------------------------------------------------------------------------------------------
ORD3_CASES = {
    "supercell3d_16x16x8": (16, 16, 8, 1, 16000., 16000., 20000., "supercell", 3, True),
    "supercell2d_64x1x32": (64, 1, 32, 1, 100000., 100000., 20000., "supercell", 3, True),
    "supercell3d_nens2_12x10x8": (12, 10, 8, 2, 6000., 5000., 20000., "supercell", 3, True),
    "city_48x48x12_nograv": (48, 48, 12, 1, 2400., 2400., 120., "city", 1, False),
}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(ORD3_CASES))
@pytest.mark.parametrize("order", [3, 7, 9])
def test_weno_orders_3_7_9(mw, oracle, name, mode, order):
    """MW_ORD = 3, 7, 9 (dynamics_euler_stratified_wenofv.h:24-28).  Orders 7 / 9: WenoLimiter<7> / <9> (hs = 3 / 4: the slabs get
    4- / 5-cell x, y halos and 3 / 4 z levels), `ord`-point GLL initial data; oracle = the restatement compiled with -DMW_ORD.
    Modes: 0 = production (order 3: the marching kernels -- 2-D, member-major nens = 2 and the immersed city configuration included;
    orders 7 / 9: the general kernels), 1 = strict (the reference's operation order), 2 = the general kernels with fast arithmetic."""
    if mode == 2 and order != 3:
        pytest.skip("orders 7 / 9: mode 0 already runs the general kernels")
    from miniweatherml_amd import modules
    O3 = oracle.with_order(order)
    nx, ny, nz, nens, xlen, ylen, zlen, init, nt, grav = ORD3_CASES[name]
    micro = None
    if nt == 1:
        class OneTracer(modules.Microphysics_Kessler):
            def init(self, coupler):
                coupler.add_tracer("water_vapor", "Water Vapor", True, True)
        micro = OneTracer()
    coupler, dycore, _ = modules.make_supercell(nx, ny, nz, nens, xlen, ylen, zlen, init, micro=micro, enable_gravity=grav,
                                                perturb=(init == "supercell"), ord=order)
    odyc, of = O3.supercell_setup(nx, ny, nz, nens, xlen, ylen, zlen, init_data=init, num_tracers=nt, enable_gravity=grav,
                                  perturb=(init == "supercell"))
    assert dycore.ord == order and dycore.hs == (order - 1) // 2
    hy = odyc.hy()
    for k in ("hy_dens_cells", "hy_dens_theta_cells", "hy_dens_edges", "hy_dens_theta_edges"):
        assert np.array_equal(getattr(dycore, k), hy[k]), k          # `ord`-point GLL columns on the host: bitwise
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-13, "ord%d init %s" % (order, name))
    push_fields(coupler, of)
    dycore.set_strict(mode)
    dt = dycore.compute_time_step(coupler)
    dycore.time_step(coupler, dt)
    odyc.time_step(of, dt)
    # Order 9: in the 2-D case ~20 cells at the rim of the warm bubble differ by up to 1.3e-11 of the field's scale after one step, in
    # both run-time modes (order 7 and every other order-9 case: <= 1e-13).  The scheme itself is that touchy there: the ORACLE run
    # from inputs with every field perturbed by one ulp (random signs) moves by 1.7e-10 of the scale in one step at order 9 and by
    # 4e-11 at orders 5 and 7 (horizontally uniform data: the candidates' total variations sit at the 1e-20 switches of `convexify`,
    # WenoLimiter_recon.h:12-15) -- the device's last-bit differences in stage 1 (pow, exp) are such a perturbation.
    tol1 = 1e-10 if order == 9 else 1e-11
    compare_fields(gpu_fields(coupler), of.as_dict(), tol1, "ord%d %s mode %d, 1 step" % (order, name, mode))
    for _ in range(9):
        dycore.time_step(coupler, dt)
        odyc.time_step(of, dt)
    compare_fields(gpu_fields(coupler), of.as_dict(), 1e-9, "ord%d %s mode %d, 10 steps" % (order, name, mode))
    # and it is not the order-5 scheme
    o5, f5 = oracle.supercell_setup(nx, ny, nz, nens, xlen, ylen, zlen, init_data=init, num_tracers=nt, enable_gravity=grav,
                                    perturb=(init == "supercell"))
    for _ in range(10):
        o5.time_step(f5, dt)
    assert np.max(np.abs(f5.uvel - of.uvel)) > 1e-6


@pytest.mark.parametrize("nranks,rank", [(1, 0), (4, 3)])
def test_random_temperature_perturbation_is_bitwise_the_oracles(mw, oracle, nranks, rank):
    """perturb_temperature(random = true) (perturb_temperature.h:25-39): +-3 K noise on the lowest nz/4 levels, one draw per (level,
    column) from a globally unique key -- with splitmix64 standing in for yakl::Random on both sides, so the two must agree bit for
    bit, also on a rank of a decomposition (the key starts at myrank * nz*nx*ny*nens) and with the thermal applied afterwards."""
    from miniweatherml_amd import modules
    nx, ny, nz, nens = 24, 20, 16, 2
    coupler, dycore, _ = modules.make_supercell(nx, ny, nz, nens, 12000., 10000., 20000., nranks=nranks, myrank=rank, perturb=False)
    odyc, of = oracle.supercell_setup(nx, ny, nz, nens, 12000., 10000., 20000., nranks=nranks, rank=rank, perturb=False)
    push_fields(coupler, of)                                      # same starting temperature on both sides
    t0 = of.temp.copy()
    modules.perturb_temperature(coupler, thermal=False, random=True)
    oracle.perturb_temperature(odyc.p, of.temp, thermal=False, random=True, myrank=rank)
    got = coupler.get_data_manager_readonly().get("temp", True).cpu().numpy()
    assert np.array_equal(got, of.temp)                           # the noise: bit for bit
    record_comparison("perturb_temperature(random = true): bit for bit the oracle's")
    push_fields(coupler, of)
    of.temp[...] = t0
    coupler.get_data_manager_readwrite().get("temp", True).copy_(torch.as_tensor(t0, device="cuda"))
    modules.perturb_temperature(coupler, thermal=True, random=True)
    oracle.perturb_temperature(odyc.p, of.temp, thermal=True, random=True, myrank=rank)
    got = coupler.get_data_manager_readonly().get("temp", True).cpu().numpy()
    assert np.max(np.abs(got - of.temp)) <= 1e-13 * 300.0         # + the thermal (device pow / cos: rounding level)
    lev = nz // 4
    d = of.temp - t0
    assert np.all(np.abs(d[:lev]) <= 3.0 + 5.0) and np.abs(d[:lev]).max() > 1.0       # noise (<= 3 K) + bubble (<= 5 K)
    only_noise = oracle.Fields(odyc.p).temp * 0
    oracle.perturb_temperature(odyc.p, only_noise, thermal=False, random=True, myrank=rank)
    assert np.all(only_noise[lev:] == 0) and np.abs(only_noise[:lev]).max() <= 3.0 and abs(only_noise[:lev].mean()) < 0.1
    if nranks > 1:                                                # another rank draws other numbers
        other = only_noise * 0
        oracle.perturb_temperature(odyc.p, other, thermal=False, random=True, myrank=0)
        assert not np.array_equal(other, only_noise)


def test_block_narrower_than_its_halo_is_refused(mw):
    """A periodic halo is filled from the interior of the same block and the strips of an exchange are HX / HY cells deep: a block
    narrower than the halo of its WENO order (3 cells up to order 5, 4 / 5 for orders 7 / 9) would read cells that are not filled
    yet.  The handle refuses instead of computing silently wrong values, and keeps its previous order."""
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd.capi import MWError
    L = capi.lib()
    coupler, dycore, micro = modules.make_supercell(4, 4, 8, 1, 2000.0, 2000.0, 20000.0, "thermal", perturb=False)
    assert L.mw_dycore_set_order(dycore.h, 9) != 0 and b"narrower than the x halo" in L.mw_last_error()
    assert L.mw_dycore_set_order(dycore.h, 7) == 0            # 4 cells wide: just fits the 4-cell halo of order 7
    dt = dycore.compute_time_step(coupler)
    dycore.time_step(coupler, dt)                             # still a working handle
    assert L.mw_dycore_set_order(dycore.h, 5) == 0
    assert L.mw_dycore_set_bc(dycore.h, 0, 0, 0) == 0         # z periodic: nz = 8 >= 2
    coupler2, dycore2, _ = modules.make_supercell(6, 6, 3, 1, 3000.0, 3000.0, 20000.0, "thermal", perturb=False)
    capi.check(L.mw_dycore_set_order(dycore2.h, 9))           # z halo 4 > nz = 3: fine with a wall ...
    assert L.mw_dycore_set_bc(dycore2.h, 0, 0, 0) != 0 and b"bc_z = periodic" in L.mw_last_error()      # ... refused with a periodic z
    with pytest.raises(MWError):
        c3, d3, _ = modules.make_supercell(6, 6, 3, 1, 3000.0, 3000.0, 20000.0, "thermal", perturb=False, ord=9)
        d3.set_bc(c3, 0, 0, 0)
