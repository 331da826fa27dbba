"""The reference drivers' set-up sequences and time-loop bodies over this host's modules:

  make_supercell, supercell_step       experiments/supercell_example/driver.cpp:41-61 and :66-79
  make_simple_city, simple_city_step   experiments/simple_city/driver.cpp:32-62 and :66-79"""
from .city import Horizontal_Sponge, Time_Averager
from .column import ColumnNudger, sponge_layer
from .coupler import Coupler
from .dycore import Dynamics_Euler_Stratified_WenoFV, perturb_temperature
from .microphysics import Microphysics_Kessler


def make_supercell(nx_glob, ny_glob, nz, nens=1, xlen=1.0e5, ylen=1.0e5, zlen=2.0e4, init_data="supercell", device="cuda:0",
                   nranks=1, myrank=0, micro=None, enable_gravity=None, perturb=True, with_nudger=False, ord=5):
    """The set-up sequence of experiments/supercell_example/driver.cpp:41-61 (column nudger excluded)."""
    coupler = Coupler(device)
    coupler.set_option("out_prefix", "test")
    coupler.set_option("init_data", init_data)
    coupler.set_option("out_freq", -1.0)
    if enable_gravity is not None:
        coupler.set_option("enable_gravity", bool(enable_gravity))
    coupler.distribute_mpi_and_allocate_coupled_state(nz, ny_glob, nx_glob, nens, nranks, myrank)
    coupler.set_grid(xlen, ylen, zlen)
    micro = micro or Microphysics_Kessler()
    dycore = Dynamics_Euler_Stratified_WenoFV(ord)
    micro.init(coupler)
    dycore.init(coupler)
    if with_nudger:
        nudger = ColumnNudger()
        nudger.set_column(coupler)                 # driver.cpp:60: set the column BEFORE perturbing
    if perturb:
        perturb_temperature(coupler)
    if with_nudger:
        return coupler, dycore, micro, nudger
    return coupler, dycore, micro


def make_simple_city(nx_glob, ny_glob, nz, nens=1, xlen=2400.0, ylen=2400.0, zlen=120.0, init_data="city", device="cuda:0",
                     nranks=1, myrank=0, out_prefix="test", ord=5):
    """The set-up sequence of experiments/simple_city/driver.cpp:32-62: only water_vapor is registered (zero), gravity off,
    dycore.init -> horiz_sponge.init(coupler, 10, 1.) -> time_averager.init."""
    coupler = Coupler(device)
    coupler.set_option("out_prefix", out_prefix)
    coupler.set_option("init_data", init_data)
    coupler.set_option("out_freq", -1.0)
    coupler.set_option("enable_gravity", False)
    coupler.distribute_mpi_and_allocate_coupled_state(nz, ny_glob, nx_glob, nens, nranks, myrank)
    coupler.set_grid(xlen, ylen, zlen)
    coupler.add_tracer("water_vapor", "water_vapor", True, True)               # driver.cpp:55-56
    coupler.get_data_manager_readwrite().get("water_vapor").zero_()
    dycore, horiz_sponge, time_averager = Dynamics_Euler_Stratified_WenoFV(ord), Horizontal_Sponge(), Time_Averager()
    dycore.init(coupler)
    horiz_sponge.init(coupler, 10, 1.0)
    time_averager.init(coupler)
    return coupler, dycore, horiz_sponge, time_averager


def simple_city_step(coupler, dycore, horiz_sponge, time_averager, dtphys=None):
    """One iteration of experiments/simple_city/driver.cpp:66-79."""
    if dtphys is None or dtphys <= 0:
        dtphys = dycore.compute_time_step(coupler)
    horiz_sponge.apply(coupler, dtphys, True, True, False, False)
    dycore.time_step(coupler, dtphys)
    sponge_layer(coupler, dtphys, 1)
    time_averager.accumulate(coupler, dtphys)
    return dtphys


def supercell_step(coupler, dycore, micro, nudger, dtphys=None, defer_nudge=False):
    """One iteration of the reference's time loop, experiments/supercell_example/driver.cpp:66-79.  defer_nudge: the nudger's increments ride
    on the next dycore step's conversion instead of a pass of their own (ColumnNudger.nudge_to_column(defer_to=...)): same bits."""
    if dtphys is None:
        dtphys = dycore.compute_time_step(coupler)
    dycore.time_step(coupler, dtphys)
    micro.time_step(coupler, dtphys)
    sponge_layer(coupler, dtphys)
    nudger.nudge_to_column(coupler, dtphys, defer_to=dycore if defer_nudge else None)
    return dtphys
