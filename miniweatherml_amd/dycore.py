"""The dynamical core and its initial perturbation (same class and method names, argument meaning and error behaviour as the
reference), thin drivers of the C ABI in include/mw_cdna4.h:

  Dynamics_Euler_Stratified_WenoFV   model/modules/dynamics_euler_stratified_wenofv.h:20-2196
  perturb_temperature                model/modules/perturb_temperature.h:8-67

No arithmetic happens in Python: everything runs in libmw_cdna4.so on the GPU (no fallback).  DEFAULT_OPTIONS and PATH_LOG are this
process's option table and dispatcher-path log: tests and tools change them in place, so they are never rebound."""
import ctypes as C
import os

import numpy as np
import torch

from . import capi
from ._ffi import _ptr, _stream_ptr
from .capi import MWError, check
from .coupler import endrun
from .ncio import dycore_output


# Options every NEW dycore handle of this process gets right after mw_dycore_create (mw_dycore_set_option; keys in include/mw_cdna4.h).
# Tests and A/B tools fill it (monkeypatch.setitem) where rounds 1-4 set MW_* environment variables; empty = the library's defaults.
DEFAULT_OPTIONS = {}
# (convenience of THIS Python host, read once at import -- the library itself never looks at it: MW_OPTIONS="pipe=0,chunk_z=7" pre-fills
#  the table for command-line A/B runs, e.g. tools/ab_bench.sh)
for _kv in filter(None, os.environ.get("MW_OPTIONS", "").split(",")):
    _k, _, _v = _kv.partition("=")
    DEFAULT_OPTIONS[_k.strip()] = int(_v)


# What the dispatcher chose in every time_step of this process since the list was last cleared (mw_dycore_path): the tests' comparisons
# drain it, so that each oracle comparison is logged with the kernel paths that produced the compared fields (tests/util.py).
PATH_LOG = []


class Dynamics_Euler_Stratified_WenoFV:
    ord = 5               # the reference's compile-time MW_ORD (:24-29); Dynamics_Euler_Stratified_WenoFV(ord=3) = its -DMW_ORD=3 build
    hs = 2
    num_state = 5
    idR, idU, idV, idW, idT = 0, 1, 2, 3, 4

    def __init__(self, ord=5):
        if ord not in (3, 5, 7, 9):
            endrun("ERROR: WENO order must be 3, 5, 7 or 9")
        self.ord, self.hs = ord, (ord - 1) // 2
        self.h = C.c_void_p(None)
        self.etime = 0.0
        self._tracer_ptrs = None
        self._fields = None

    def __del__(self):
        try:
            if self.h and self.h.value:
                capi.lib().mw_dycore_destroy(self.h)
                self.h = C.c_void_p(None)
        except Exception:
            pass

    # dynamics_euler_stratified_wenofv.h:70-77
    def compute_time_step(self, coupler):
        return capi.lib().mw_dycore_compute_time_step(C.byref(coupler.grid))

    def _bind(self, coupler):
        dm = coupler.get_data_manager_readwrite()
        names = coupler.get_tracer_names()
        self._fields = [dm.get(n) for n in ("density_dry", "uvel", "vvel", "wvel", "temp")]
        self._tracers = [dm.get(n) for n in names]
        arr = (C.c_void_p * max(1, len(names)))()
        for i, t in enumerate(self._tracers):
            arr[i] = _ptr(t).value
        self._tracer_ptrs = arr

    # dynamics_euler_stratified_wenofv.h:1197-1683
    def init(self, coupler):
        L = capi.lib()
        g = coupler.grid
        nz, ny, nx, nens = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()
        # physical constants only if absent (:1227-1249)
        gc = capi.Grid()
        check(L.mw_default_constants(C.byref(gc)))
        for k in ("R_d", "cp_d", "R_v", "cp_v", "p0", "grav", "earthrot"):
            if not coupler.option_exists(k):
                coupler.set_option(k, getattr(gc, k))
        R_d, cp_d, p0 = coupler.get_option("R_d"), coupler.get_option("cp_d"), coupler.get_option("p0")
        if not coupler.option_exists("cv_d"): coupler.set_option("cv_d", cp_d - R_d)
        if not coupler.option_exists("gamma_d"): coupler.set_option("gamma_d", cp_d / coupler.get_option("cv_d"))
        if not coupler.option_exists("kappa_d"): coupler.set_option("kappa_d", R_d / cp_d)
        if not coupler.option_exists("cv_v"): coupler.set_option("cv_v", coupler.get_option("R_v") - coupler.get_option("cp_v"))
        if not coupler.option_exists("C0"):
            coupler.set_option("C0", gc.C0 if (R_d, cp_d, p0) == (gc.R_d, gc.cp_d, gc.p0) else
                               float(np.power(R_d * np.power(p0, -coupler.get_option("kappa_d")), coupler.get_option("gamma_d"))))
        coupler.set_option("latitude", 0.0)
        for k in ("R_d", "R_v", "cp_d", "cp_v", "p0", "grav", "gamma_d", "kappa_d", "C0", "earthrot", "latitude"):
            setattr(g, k, float(coupler.get_option(k)))
        dm = coupler.get_data_manager_readwrite()
        for n in ("density_dry", "uvel", "vvel", "wvel", "temp"):            # :1253-1257
            dm.register_and_allocate(n, "", (nz, ny, nx, nens))
        names = coupler.get_tracer_names()
        T = len(names)
        if "water_vapor" not in names:
            endrun("ERROR: a tracer named water_vapor must be registered before dycore.init (idWV, :1292)")
        pos = bytes(int(coupler.get_tracer_info(n)[2]) for n in names)
        adds = bytes(int(coupler.get_tracer_info(n)[3]) for n in names)
        g.num_tracers = T
        g.idWV = names.index("water_vapor")
        coupler.set_option("idWV", g.idWV)                                     # :1300
        dm.register_and_allocate("tracer_adds_mass", "", (T,), dtype=torch.bool)
        dm.get("tracer_adds_mass").copy_(torch.tensor([b != 0 for b in adds]))
        init_data = coupler.get_option("init_data")
        self.out_freq = coupler.get_option("out_freq", -1.0)
        if init_data not in capi.INIT_IDS:
            endrun("ERROR: Invalid init_data in yaml input file")              # :1310
        g.enable_gravity = int(bool(coupler.get_option("enable_gravity", True)))
        g.bc_x, g.bc_y, g.bc_z, g.use_immersed = capi.BC_PERIODIC, capi.BC_PERIODIC, capi.BC_WALL, 0
        with torch.cuda.device(coupler.device):
            check(L.mw_dycore_create(C.byref(self.h), C.byref(g), pos, adds, _stream_ptr(coupler.device)))
            for key, val in DEFAULT_OPTIONS.items():
                self.set_option(key, val)
            if self.ord != 5:
                check(L.mw_dycore_set_order(self.h, self.ord))              # before init: the supercell data uses `ord` GLL points
            self._bind(coupler)
            check(L.mw_dycore_init(self.h, capi.INIT_IDS[init_data], *[_ptr(t) for t in self._fields], self._tracer_ptrs))
        check(L.mw_dycore_get_grid(self.h, C.byref(g)))
        coupler.set_option("use_immersed_boundaries", bool(g.use_immersed))    # :1312,1426,1554
        coupler.add_option("bc_x", g.bc_x); coupler.add_option("bc_y", g.bc_y); coupler.add_option("bc_z", g.bc_z)
        # fields the reference registers for other modules (:1313, :1663-1682) -- zero-copy views of the handle's memory
        hy = [np.zeros((nz, nens)), np.zeros((nz, nens)), np.zeros((nz + 1, nens)), np.zeros((nz + 1, nens))]
        check(L.mw_dycore_get_background(self.h, *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in hy]))
        self.hy_dens_cells, self.hy_dens_theta_cells, self.hy_dens_edges, self.hy_dens_theta_edges = hy
        dm.register_and_allocate("hy_dens_cells", "hydrostatic density cell averages", (nz, nens)).copy_(torch.from_numpy(hy[0]))
        dm.register_and_allocate("hy_dens_theta_cells", "hydrostatic density*theta cell averages", (nz, nens)).copy_(torch.from_numpy(hy[1]))
        self.etime = 0.0
        self.num_out = 0
        if self.out_freq >= 0.0:                                               # :1659: the initial state is record 0
            self.output(coupler, self.etime)

    def _wrap(self, ptr, shape):
        """Zero-copy CUDA tensor over library-owned device memory."""
        n = int(np.prod(shape))

        class _Arr:
            pass
        a = _Arr()
        a.__cuda_array_interface__ = dict(shape=(n,), typestr="<f8", data=(int(ptr), False), version=2)
        return torch.as_tensor(a, device="cuda").view(*shape)

    def fluxes(self, coupler):
        """state_flux_{x,y,z}, tracers_flux_{x,y,z} as the reference registers them (:1671-1676)."""
        out = (C.c_void_p * 6)()
        check(capi.lib().mw_dycore_get_fluxes(self.h, out))
        nz, ny, nx, nens, T = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens(), coupler.get_num_tracers()
        shp = [(5, nz, ny, nx + 1, nens), (5, nz, ny + 1, nx, nens), (5, nz + 1, ny, nx, nens),
               (T, nz, ny, nx + 1, nens), (T, nz, ny + 1, nx, nens), (T, nz + 1, ny, nx, nens)]
        names = ["state_flux_x", "state_flux_y", "state_flux_z", "tracers_flux_x", "tracers_flux_y", "tracers_flux_z"]
        with torch.cuda.device(coupler.device):
            return {n: self._wrap(out[i], shp[i]) for i, n in enumerate(names)}

    def immersed_proportion(self, coupler):
        p = capi.lib().mw_dycore_immersed_proportion(self.h)
        with torch.cuda.device(coupler.device):
            return self._wrap(p, (coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens()))

    # dynamics_euler_stratified_wenofv.h:81-198 (file output excluded)
    def time_step(self, coupler, dt_phys):
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_dycore_time_step(self.h, *[_ptr(t) for t in self._fields], self._tracer_ptrs, float(dt_phys)))
        self._parked = False                                    # (parked column increments were consumed by the conversion, or applied at entry)
        self.etime += dt_phys
        PATH_LOG.append(self.path())
        if len(PATH_LOG) > 4096:                                # (a long run that nobody drains: keep the distinct entries)
            PATH_LOG[:] = sorted(set(PATH_LOG))
        # :183-186.  out_freq == 0: the reference's etime/0. is +inf >= num_out+1, i.e. a record after every step
        if self.out_freq >= 0.0 and (self.out_freq == 0.0 or self.etime / self.out_freq >= self.num_out + 1):
            self.output(coupler, self.etime)
            self.num_out += 1

    # one compute_tendencies(state(coupler), dt) (:204-552): returns (state_tend, tracers_tend); fluxes via .fluxes()
    def compute_tendencies(self, coupler, dt):
        nz, ny, nx, nens, T = coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens(), coupler.get_num_tracers()
        st = torch.zeros((5, nz, ny, nx, nens), dtype=torch.float64, device=coupler.device)
        tt = torch.zeros((T, nz, ny, nx, nens), dtype=torch.float64, device=coupler.device)
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_dycore_compute_tendencies(self.h, *[_ptr(t) for t in self._fields], self._tracer_ptrs, float(dt),
                                                          _ptr(st), _ptr(tt)))
        return st, tt

    def set_strict(self, strict):
        check(capi.lib().mw_dycore_set_strict(self.h, int(strict)))

    def set_option(self, key, value):
        """A run-time option of this handle (mw_dycore_set_option: schedule, kernel forms, chunk sizes, transport; include/mw_cdna4.h)."""
        check(capi.lib().mw_dycore_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_longlong(0)
        check(capi.lib().mw_dycore_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    _parked = False       # column increments may be parked in the handle (set by ColumnNudger.nudge_to_column(defer_to=self), cleared by time_step / flush)

    def flush_pending(self):
        """Applies column increments that ColumnNudger.nudge_to_column(..., defer_to=self) parked in this handle (mw_dycore_flush_pending); a
        no-op when there are none.  The coupler's DataManager calls it in front of every field access."""
        if self._parked:
            self._parked = False
            check(capi.lib().mw_dycore_flush_pending(self.h))

    def pending(self):
        """(parked now, [rode on a conversion, applied by a pass]) -- mw_dycore_pending."""
        out = (C.c_ulonglong * 2)()
        return bool(capi.lib().mw_dycore_pending(self.h, out)), [int(out[0]), int(out[1])]

    def zero_violations(self):
        """(total, [4]) of option zero_verify's counters (mw_debug_zero_violations; a test aid): claims of the zero-row maps that the data
        contradicted; total = -1 when the option never ran on this handle."""
        out = (C.c_ulonglong * 4)()
        n = capi.lib().mw_debug_zero_violations(self.h, out)
        return n, [int(v) for v in out]

    def vapour_redo(self):
        """How many RK stages of the last time step redid their water vapour in the tracer stage's three-tracer form (mw_debug_vapour_redo; a
        test aid of option vapour_state)."""
        return int(capi.lib().mw_debug_vapour_redo(self.h))

    def tracer_flags(self):
        """The fused tracer stage's per-cell flag bytes as its last launch left them (mw_debug_tracer_flags; a test aid): uint8, cell (k, j, x) at (k * ny + j) * nx * nens + x."""
        n = int(capi.lib().mw_debug_tracer_flags(self.h, None, 0))
        buf = np.zeros(max(n, 0), dtype=np.uint8)
        if n < 0 or capi.lib().mw_debug_tracer_flags(self.h, buf.ctypes.data_as(C.c_void_p), n) != n:
            raise MWError("mw_debug_tracer_flags failed")
        return buf

    def set_bc(self, coupler, bc_x, bc_y, bc_z):
        check(capi.lib().mw_dycore_set_bc(self.h, bc_x, bc_y, bc_z))
        coupler.set_option("bc_x", bc_x); coupler.set_option("bc_y", bc_y); coupler.set_option("bc_z", bc_z)

    def schedule(self):
        """What the last time_step ran (mw_dycore_schedule): dict(streams = "one" | "two" | "pipelined", y_all, general_kernels)."""
        v = capi.lib().mw_dycore_schedule(self.h)
        return dict(code=v, streams=("one stream", "two streams (state | tracers, tracer stream at high priority)",
                                     "one compute stream, strip exchange on a side stream beside the inner y rows / the tracer stage")[v & 3],
                    y_all=bool(v & 4), general_kernels=bool(v & 8))

    def path(self):
        """The dispatcher's decisions of the last time_step, spelled out (mw_dycore_path)."""
        return (capi.lib().mw_dycore_path(self.h) or b"").decode()

    def rccl_info(self):
        """(ranks, rank, lanes) as the installed RCCL transport's communicator reports them (ncclCommCount / ncclCommUserRank)."""
        n, r, l = C.c_int(-1), C.c_int(-1), C.c_int(0)
        check(capi.lib().mw_dycore_rccl_info(self.h, C.byref(n), C.byref(r), C.byref(l)))
        return n.value, r.value, l.value

    def profile(self, enable):
        check(capi.lib().mw_dycore_profile(self.h, int(enable)))

    def profile_get(self, which):
        ms, n = C.c_double(), C.c_longlong()
        check(capi.lib().mw_dycore_profile_get(self.h, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # dynamics_euler_stratified_wenofv.h:2019-2191
    def output(self, coupler, etime, **kw):
        return dycore_output(coupler, etime, **kw)


def perturb_temperature(coupler, thermal=True, random=False):                   # perturb_temperature.h:8-67
    temp = coupler.get_data_manager_readwrite().get("temp")
    with torch.cuda.device(coupler.device):
        if random:      # :25-39 (splitmix64 in place of the unavailable yakl::Random, see include/mw_cdna4.h)
            check(capi.lib().mw_perturb_temperature_random(C.byref(coupler.grid), _ptr(temp), _stream_ptr(coupler.device)))
        if thermal:     # :41-66
            check(capi.lib().mw_perturb_temperature(C.byref(coupler.grid), _ptr(temp), _stream_ptr(coupler.device)))
