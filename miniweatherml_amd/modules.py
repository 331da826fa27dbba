"""Host-side mirror of the reference *modules* for the hot path (same class names, method names, argument
meaning, error behaviour), each a thin driver of the C ABI in include/mw_cdna4.h:

  Dynamics_Euler_Stratified_WenoFV   model/modules/dynamics_euler_stratified_wenofv.h:20-2196
  Microphysics_Kessler               model/modules/microphysics_kessler.h:8-346
  Microphysics_Kessler_Surrogate     experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h
  perturb_temperature                model/modules/perturb_temperature.h:8-67

No arithmetic happens in Python: everything runs in libmw_cdna4.so on the GPU (no fallback).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import capi
from .capi import MWError, check
from .coupler import Coupler, endrun

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def _ptr(t):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise MWError("field tensors must be contiguous fp64 CUDA tensors")
    return C.c_void_p(t.data_ptr())


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


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


class Microphysics_Kessler:
    num_tracers = 3
    ID_V, ID_C, ID_R = 0, 1, 2

    def __init__(self):                                                        # microphysics_kessler.h:29-41
        self.R_d, self.cp_d = 287., 1003.
        self.cv_d = self.cp_d - self.R_d
        self.gamma_d = self.cp_d / self.cv_d
        self.kappa_d = self.R_d / self.cp_d
        self.R_v, self.cp_v = 461., 1859.
        self.cv_v = self.R_v - self.cp_v
        self.p0, self.grav = 1.e5, 9.81
        self._ws = None
        self.strict = 0          # 1: the strict path (reference operation order, glibc's pow / exp): bit-identical to the CPU oracle

    def set_strict(self, strict):
        self.strict = int(bool(strict))

    @staticmethod
    def get_num_tracers():
        return 3

    def micro_name(self):
        return "kessler"

    def init(self, coupler):                                                   # :51-96
        coupler.add_tracer("water_vapor", "Water Vapor", True, True)
        coupler.add_tracer("cloud_liquid", "Cloud liquid", True, True)
        coupler.add_tracer("precip_liquid", "precip_liquid", True, True)
        dm = coupler.get_data_manager_readwrite()
        dm.register_and_allocate("precl", "precipitation rate", (coupler.get_ny(), coupler.get_nx(), coupler.get_nens()),
                                 ["y", "x", "nens"])
        coupler.set_option("micro", "kessler")
        for k in ("R_d", "cp_d", "cv_d", "gamma_d", "kappa_d", "R_v", "cp_v", "cv_v", "p0", "grav"):
            coupler.set_option(k, getattr(self, k))

    def time_step(self, coupler, dt, return_rainsplit=False):                  # :99-162
        dm = coupler.get_data_manager_readwrite()
        rho_v, rho_c, rho_r = dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid")
        rho_d, temp, precl = dm.get("density_dry", readonly=True), dm.get("temp"), dm.get("precl")
        nz = coupler.get_nz()
        ncol = coupler.get_ny() * coupler.get_nx() * coupler.get_nens()
        L = capi.lib()
        nbytes = L.mw_kessler_workspace_bytes(nz, ncol)
        if self._ws is None or self._ws.numel() * 8 < nbytes:
            self._ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=coupler.device)
        rs = C.c_int(0)
        check(L.mw_kessler_set_strict(self.strict))
        with torch.cuda.device(coupler.device):
            check(L.mw_kessler_time_step(nz, ncol, coupler.get_dz(), float(dt), _ptr(rho_v), _ptr(rho_c), _ptr(rho_r), _ptr(rho_d),
                                         _ptr(temp), _ptr(precl), _ptr(self._ws), C.byref(rs) if return_rainsplit else None,
                                         _stream_ptr(coupler.device)))
        return rs.value if return_rainsplit else None


def load_h5_weights(fname, group, dataset):
    """ponni::load_h5_weights<N> (microphysics_kessler_ponni.h:103-107): one float32 dataset of a Keras HDF5 weight file, through the
    library's dependency-free reader (mw_h5.cpp)."""
    L = capi.lib()
    dims, nd = (C.c_longlong * 8)(), C.c_int(0)
    fb, gb, db = str(fname).encode(), group.encode(), dataset.encode()
    check(L.mw_h5_read_f32(fb, gb, db, None, 0, dims, C.byref(nd)))
    shape = tuple(int(dims[i]) for i in range(nd.value))
    out = np.empty(shape, dtype=np.float32)
    check(L.mw_h5_read_f32(fb, gb, db, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, dims, C.byref(nd)))
    return out


def load_surrogate_weights(weights_txt=None, in_scaling_txt=None, out_scaling_txt=None, weights_h5=None):
    """The Keras weights + min/max scaling tables (microphysics_kessler_ponni.h:97-135).  weights_h5: the reference's
    `keras_weights_h5` file, read like ponni::load_h5_weights does (:103-107); weights_txt: a text export of the 104 values
    (tools/export_mlp_weights.sh).  Default: the reference's shipped weight file (miniweatherml_amd/data/).
    The model is inferred from the text files: 5 scaling rows + 104 weights = the single-cell model (W1 (5,10)), 9 rows + 144 weights = the
    two-cell stencil model (W1 (9,10); surrogate_train --stencil).  Any other pairing is refused; so is an .h5 file of a stencil model."""
    if weights_txt is None and weights_h5 is None:
        weights_h5 = os.path.join(_DATA, "supercell_kessler_singlecell_model_weights.h5")
    if weights_h5 is not None:
        W1 = load_h5_weights(weights_h5, "/dense_6/dense_6", "kernel:0")       # Matvec 1   (in, out) = (5, 10)
        b1 = load_h5_weights(weights_h5, "/dense_6/dense_6", "bias:0")
        W2 = load_h5_weights(weights_h5, "/dense_7/dense_7", "kernel:0")       # Matvec 2   (10, 4)
        b2 = load_h5_weights(weights_h5, "/dense_7/dense_7", "bias:0")
        if W1.shape != (5, 10) or b1.shape != (10,) or W2.shape != (10, 4) or b2.shape != (4,):
            endrun("surrogate weight file: expected Dense(5->10) and Dense(10->4) (an .h5 file of the stencil model is not supported: "
                   "use the text files surrogate_train writes)")
        nw = 104
    else:
        w = np.loadtxt(weights_txt, dtype=np.float64, comments="#").astype(np.float32).ravel()
        nw = w.size
    scl_in = np.atleast_2d(np.loadtxt(in_scaling_txt or os.path.join(_DATA, "kessler_surrogate_input_scaling.txt")))
    rows = scl_in.shape[0] if scl_in.shape[1:] == (2,) else -1
    if (rows, nw) not in ((5, 104), (9, 144)):
        endrun("surrogate files: %d input scaling rows with %d weights; expected 5 rows + 104 weights (single-cell model) or 9 rows + 144 "
               "weights (stencil model)" % (rows if rows >= 0 else scl_in.size // 2, nw))
    if weights_h5 is None:
        a = 10 * rows
        W1, b1, W2, b2 = w[:a].reshape(rows, 10).copy(), w[a:a + 10].copy(), w[a + 10:a + 50].reshape(10, 4).copy(), w[a + 50:a + 54].copy()
    scl_out = np.loadtxt(out_scaling_txt or os.path.join(_DATA, "kessler_surrogate_output_scaling.txt")).reshape(4, 2)
    return W1, b1, W2, b2, np.ascontiguousarray(scl_in), np.ascontiguousarray(scl_out)


def mlp_forward(temp, rho_d, rho_v, rho_c, rho_r, W1, b1, W2, b2, scl_in, scl_out, outs=None, strict=0):
    """model.forward_batch_parallel with the fused scaling (microphysics_kessler_ponni.h:176-202).  strict = 1: the thread-per-cell
    form that accumulates in index order (bit-identical to the CPU restatement) instead of the MFMA kernels."""
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    if outs is None:
        outs = [torch.empty_like(temp) for _ in range(4)]
    check(capi.lib().mw_mlp_set_strict(int(bool(strict))))
    with torch.cuda.device(temp.device):
        check(capi.lib().mw_mlp_forward(temp.numel(), _ptr(temp), _ptr(rho_d), _ptr(rho_v), _ptr(rho_c), _ptr(rho_r),
                                        W1.ctypes.data_as(fp), b1.ctypes.data_as(fp), W2.ctypes.data_as(fp), b2.ctypes.data_as(fp),
                                        scl_in.ctypes.data_as(dp), scl_out.ctypes.data_as(dp), *[_ptr(o) for o in outs],
                                        _stream_ptr(temp.device)))
    return outs


def mlp_stencil_forward(nz, temp, rho_d, rho_v, rho_c, rho_r, W1, b1, W2, b2, scl_in, scl_out, outs=None, strict=0):
    """mlp_forward for the two-cell stencil model (W1 (9,10), scl_in (9,2)): the fields are whole coupler arrays (nz, ...) and features
    5..8 come from level min(nz - 1, k + 1) of the same column (stencil_features states the order).  The outputs never alias the inputs."""
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    if W1.shape != (9, 10) or scl_in.shape != (9, 2):
        endrun("mlp_stencil_forward: W1 must be (9, 10) and scl_in (9, 2), got %r and %r" % (W1.shape, scl_in.shape))
    if temp.numel() % int(nz) != 0:
        endrun("mlp_stencil_forward: %d cells are not a whole number of columns of nz = %d" % (temp.numel(), nz))
    if outs is None:
        outs = [torch.empty_like(temp) for _ in range(4)]
    check(capi.lib().mw_mlp_set_strict(int(bool(strict))))
    with torch.cuda.device(temp.device):
        check(capi.lib().mw_mlp_stencil_forward(int(nz), temp.numel() // int(nz), _ptr(temp), _ptr(rho_d), _ptr(rho_v), _ptr(rho_c), _ptr(rho_r),
                                                W1.ctypes.data_as(fp), b1.ctypes.data_as(fp), W2.ctypes.data_as(fp), b2.ctypes.data_as(fp),
                                                scl_in.ctypes.data_as(dp), scl_out.ctypes.data_as(dp), *[_ptr(o) for o in outs],
                                                _stream_ptr(temp.device)))
    return outs


def stencil_features(fields, nz):
    """The nine inputs of the stencil model on the host (pure numpy): fields = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid),
    arrays whose first axis is the nz levels (any trailing shape: (ny, nx, nens) or flat columns).  Returns (9, ncells) in C order of the
    fields: rows 0..4 the cell's five, rows 5..8 temp, water_vapor, cloud_liquid, precip_liquid of level min(nz - 1, k + 1) of the same
    column and ensemble member (DataGenerator's inputs(:, :, 0) and inputs(:, 0:4, 1))."""
    f = [np.asarray(a).reshape(int(nz), -1) for a in fields]
    if len(f) != 5 or any(a.shape != f[0].shape for a in f):
        endrun("stencil_features: five fields of one shape (nz, ...) expected")
    up = np.minimum(np.arange(int(nz)) + 1, int(nz) - 1)
    rows = f + [f[i][up] for i in (0, 2, 3, 4)]
    return np.stack([r.reshape(-1) for r in rows])


class _PonniLayer(C.Structure):
    """mw_ponni_layer_t"""
    _fields_ = [("kind", C.c_int), ("n_in", C.c_int), ("n_out", C.c_int), ("negative_slope", C.c_float), ("offset", C.c_int)]


def ponni_forward(layers, x, strict=0):
    """ponni::Inference::forward_batch_parallel (microphysics_kessler_ponni.h:189) for a stack of ponni layers on a float32 CUDA tensor
    x of shape (num_in, batch), batch fastest -> (num_out, batch).  layers: ("matvec", W (in, out)) | ("bias", b) | ("relu", n, slope)
    in the order of ponni::create_inference_model's arguments (:109).  The C++ mirror is miniweatherml_amd/host/mw_ponni.h."""
    recs, params = [], []
    for l in layers:
        kind = {"matvec": 0, "bias": 1, "relu": 2}[l[0]]
        off = sum(p.size for p in params)
        if kind == 0:
            W = np.ascontiguousarray(l[1], dtype=np.float32); params.append(W.ravel()); recs.append((0, W.shape[0], W.shape[1], 0.0, off))
        elif kind == 1:
            b = np.ascontiguousarray(l[1], dtype=np.float32); params.append(b.ravel()); recs.append((1, b.size, b.size, 0.0, off))
        else:
            recs.append((2, int(l[1]), int(l[1]), float(l[2]) if len(l) > 2 else 0.0, off))
    arr = (_PonniLayer * len(recs))(*[_PonniLayer(*r) for r in recs])
    flat = np.concatenate(params).astype(np.float32) if params else np.zeros(1, np.float32)
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
        endrun("ponni_forward: x must be a contiguous float32 (num_in, batch) tensor")
    out = torch.empty((recs[-1][2], x.shape[1]), dtype=torch.float32, device=x.device)
    check(capi.lib().mw_mlp_set_strict(int(bool(strict))))
    with torch.cuda.device(x.device):
        rc = capi.lib().mw_ponni_forward(C.cast(arr, C.c_void_p), len(recs), flat.ctypes.data_as(C.POINTER(C.c_float)),
                                         int(sum(p.size for p in params)), x.shape[1], C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()),
                                         _stream_ptr(x.device))
    check(capi.lib().mw_mlp_set_strict(0))
    check(rc)
    return out


class Microphysics_Kessler_Surrogate(Microphysics_Kessler):
    """custom_modules::Microphysics_Kessler of the surrogate experiment: NN inference beside the true Kessler
    (microphysics_kessler_ponni.h:149-278).  The NN result is returned (and diffed) but not written back,
    exactly like the reference with lines :273-276 commented out."""

    online = False        # True = the four deep_copy_to lines :273-276 un-commented: the NN result replaces Kessler's
    mlp_strict = 0        # 1: the thread-per-cell MLP that accumulates in index order (bit-identical to the CPU restatement; tests)

    want_range = False    # with a committee: time_step also fills last_range, the four fields of the members' spread
    last_range = None

    def init(self, coupler, weights_txt=None, in_scaling_txt=None, out_scaling_txt=None, weights_h5=None, committee=None):
        """committee: a list of 1 .. 16 (W1, b1, W2, b2, scl_in, scl_out) tuples of one width (load_surrogate_weights' form).  The network's
        result is then the committee's mean (SurrogateBank.committee_apply), and the weight file arguments are not read."""
        super().init(coupler)
        self._nn_out = None
        self._committee = None
        if committee is not None:
            committee = list(committee)
            if any(k is not None for k in (weights_txt, in_scaling_txt, out_scaling_txt, weights_h5)):
                endrun("Microphysics_Kessler_Surrogate: a committee brings its own weights and scaling tables: give no file beside it")
            if not 1 <= len(committee) <= capi.MW_COMMITTEE_MAX_MODELS:
                endrun("Microphysics_Kessler_Surrogate: a committee has 1 to %d models, got %d" % (capi.MW_COMMITTEE_MAX_MODELS, len(committee)))
            self._committee = SurrogateBank(committee, coupler.device)
            self.W1, self.b1, self.W2, self.b2, self.scl_in, self.scl_out = committee[0]
            return
        self.W1, self.b1, self.W2, self.b2, self.scl_in, self.scl_out = load_surrogate_weights(weights_txt, in_scaling_txt,
                                                                                              out_scaling_txt, weights_h5)

    def time_step(self, coupler, dt):
        dm = coupler.get_data_manager_readwrite()
        temp, rho_d = dm.get("temp"), dm.get("density_dry", readonly=True)
        rho_v, rho_c, rho_r = dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid")
        if getattr(self, "_committee", None) is not None:
            if self._nn_out is None:
                self._nn_out = [torch.empty_like(temp) for _ in range(4)]
            if self.want_range and self.last_range is None:
                self.last_range = [torch.empty_like(temp) for _ in range(4)]
            self._committee.strict = self.mlp_strict
            # the coupler's fields are (nz, ny, nx, nens): every member is one more column, so the whole array is one member of nens = 1
            flat = [t.reshape(coupler.get_nz(), -1, 1) for t in (temp, rho_d, rho_v, rho_c, rho_r)]
            self._committee.committee_apply(coupler.get_nz(), range(self._committee.models), 0, flat,
                                            [t.reshape(coupler.get_nz(), -1, 1) for t in self._nn_out],
                                            [t.reshape(coupler.get_nz(), -1, 1) for t in self.last_range] if self.want_range else None)
        elif self.W1.shape[0] == 9:                                            # the stencil model: what load_surrogate_weights found
            self._nn_out = mlp_stencil_forward(coupler.get_nz(), temp, rho_d, rho_v, rho_c, rho_r, self.W1, self.b1, self.W2, self.b2,
                                               self.scl_in, self.scl_out, self._nn_out, strict=self.mlp_strict)
        else:
            self._nn_out = mlp_forward(temp, rho_d, rho_v, rho_c, rho_r, self.W1, self.b1, self.W2, self.b2, self.scl_in, self.scl_out,
                                       self._nn_out, strict=self.mlp_strict)
        super().time_step(coupler, dt)
        if self.online:                                                        # :273-276
            self._diffs = self.mean_diffs(coupler)                             # (the prints of :266-269 come first)
            for dst, src in zip((temp, rho_v, rho_c, rho_r), self._nn_out):
                dst.copy_(src)
        return self._nn_out            # (temp_tmp, rho_v_tmp, rho_c_tmp, rho_r_tmp)

    def mean_diffs(self, coupler):
        """The four 'Relative diff' prints (:266-269): mean(NN - Kessler)."""
        dm = coupler.get_data_manager_readonly()
        t, v, c, r = self._nn_out
        if getattr(self, "_ws_mean", None) is None:
            self._ws_mean = torch.empty(1024, dtype=torch.float64, device=coupler.device)
        out = {}
        with torch.cuda.device(coupler.device):
            for key, nn, name in (("rho_v", v, "water_vapor"), ("rho_c", c, "cloud_liquid"), ("rho_r", r, "precip_liquid"), ("temp", t, "temp")):
                m = C.c_double(0.0)
                check(capi.lib().mw_mean_diff(nn.numel(), _ptr(nn), _ptr(dm.get(name, True)), _ptr(self._ws_mean), C.byref(m),
                                              _stream_ptr(coupler.device)))
                out[key] = m.value
        return out


# ---- in-loop evaluation of candidate surrogates (mw_surrogate_eval) ---------------------------------------------------------------
EVAL_FIELDS = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")
EVAL_CLASSES = ("inactive", "active")
_EXACT_ONE = 1 << 1074            # sums are kept as integers in units of 2^-1074, the spacing of the smallest doubles: exact addition


def load_surrogate_bank(entries):
    """The models of a `surrogate_models:` list (dicts with keras_weights_txt | keras_weights_h5, nn_input_scaling, nn_output_scaling; `name`
    and other keys are ignored) as the list of load_surrogate_weights tuples that SurrogateBank takes."""
    return [load_surrogate_weights(weights_txt=e.get("keras_weights_txt"), in_scaling_txt=e.get("nn_input_scaling"),
                                   out_scaling_txt=e.get("nn_output_scaling"), weights_h5=e.get("keras_weights_h5")) for e in entries]


class SurrogateBank:
    """mw_surrogate_bank_t: K candidate networks of one width (all single-cell or all stencil), each with its own scaling tables, uploaded
    once to `device`; evaluate() refuses fields of another device.  models: a list of (W1, b1, W2, b2, scl_in, scl_out) as
    load_surrogate_weights returns them."""

    def __init__(self, models, device="cuda:0"):
        self._h = None
        self.device = torch.device(device)
        models = list(models)
        if len(models) < 1:
            endrun("SurrogateBank: no models")
        if len(models) > capi.MW_SURROGATE_MAX_MODELS:
            endrun("SurrogateBank: %d models, at most %d fit one bank" % (len(models), capi.MW_SURROGATE_MAX_MODELS))
        widths = sorted({int(np.asarray(m[0]).shape[0]) for m in models})
        if len(widths) != 1:
            endrun("SurrogateBank: models of different widths (%s inputs) cannot share a bank: one bank per width" % ", ".join(map(str, widths)))
        self.n_in, self.models = widths[0], len(models)
        a = 10 * self.n_in
        for W1, b1, W2, b2, si, so in models:
            if np.shape(W1) != (self.n_in, 10) or np.shape(b1) != (10,) or np.shape(W2) != (10, 4) or np.shape(b2) != (4,) or \
                    np.shape(si) != (self.n_in, 2) or np.shape(so) != (4, 2):
                endrun("SurrogateBank: a model is not Dense(%d->10), Dense(10->4) with (%d, 2) and (4, 2) scaling tables" % (self.n_in, self.n_in))
        params = np.ascontiguousarray([np.concatenate([np.ravel(m[0]), np.ravel(m[1]), np.ravel(m[2]), np.ravel(m[3])]) for m in models], dtype=np.float32)
        scl_in = np.ascontiguousarray([m[4] for m in models], dtype=np.float64)
        scl_out = np.ascontiguousarray([m[5] for m in models], dtype=np.float64)
        h = C.c_void_p()
        if capi.lib().mw_device_count() < 1:
            endrun("SurrogateBank: no HIP device available: libmw_cdna4 has no CPU fallback")
        with torch.cuda.device(self.device):                              # the handle's allocations live on the current device
            check(capi.lib().mw_surrogate_bank_create(C.byref(h), self.n_in, self.models, params.ctypes.data_as(C.POINTER(C.c_float)),
                                                      scl_in.ctypes.data_as(C.POINTER(C.c_double)), scl_out.ctypes.data_as(C.POINTER(C.c_double))))
        self._h = h
        self.group = int(capi.lib().mw_surrogate_eval_group(h))           # models per pass over the state
        self.strict = 0                                                   # 1: the thread-per-cell kernels (mw_mlp_set_strict)
        self._buf = None

    def __del__(self):
        try:                                                              # (at interpreter exit the module's globals may be gone)
            if getattr(self, "_h", None):
                with torch.cuda.device(self.device):
                    capi.lib().mw_surrogate_bank_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def evaluate(self, nz, in5, truth4):
        """in5: the five fields before the microphysics call (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), truth4: the four
        after it (EVAL_FIELDS); fp64 CUDA tensors of nz levels.  Returns (stats, counts): the raw (K + 1, 2, 4, 4) fp64 array
        [model | persistence][inactive, active][field][sum d, sum |d|, sum d^2, max |d|], d = prediction - truth, and the int64 cells per
        class -- one device-to-host copy for both."""
        if len(in5) != 5 or len(truth4) != 4:
            endrun("SurrogateBank.evaluate: five input fields and four truth fields expected")
        n = in5[0].numel()
        if int(nz) < 1 or n % int(nz) != 0 or any(t.numel() != n for t in list(in5) + list(truth4)):
            endrun("SurrogateBank.evaluate: the nine fields must have one size, a whole number of columns of nz = %d levels" % nz)
        dev = self.device
        if any(t.device != dev for t in list(in5) + list(truth4)):
            endrun("SurrogateBank.evaluate: the bank lives on %s, the fields on %s" % (dev, sorted({str(t.device) for t in list(in5) + list(truth4)})))
        nout = (self.models + 1) * 32
        if self._buf is None:
            self._buf = torch.empty(nout + 2, dtype=torch.int64, device=dev)                  # the statistics' bytes, then the two counts
        check(capi.lib().mw_mlp_set_strict(int(bool(self.strict))))
        with torch.cuda.device(dev):
            rc = capi.lib().mw_surrogate_eval(self._h, int(nz), n // int(nz), _field_ptr_array(in5), _field_ptr_array(truth4),
                                              C.c_void_p(self._buf.data_ptr()), C.c_void_p(self._buf.data_ptr() + 8 * nout), _stream_ptr(dev))
        check(capi.lib().mw_mlp_set_strict(0))
        check(rc)
        host = self._buf.cpu().numpy()
        return host[:nout].view(np.float64).reshape(self.models + 1, 2, 4, 4).copy(), host[nout:].copy()

    def members_apply(self, nz, members, fields5):
        """mw_surrogate_members_apply: model j of the bank replaces temp and the three water fields of ensemble member members[j] of the
        coupler's member-fastest arrays fields5 = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), each (nz, ..., nens), in
        place, with the bits the forward kernels write for that member's own values (self.strict = 1: the thread-per-cell form)."""
        members = [int(m) for m in members]
        if len(members) != self.models:
            endrun("SurrogateBank.members_apply: %d members for %d models" % (len(members), self.models))
        if len(fields5) != 5 or any(t.shape != fields5[0].shape for t in fields5) or fields5[0].dim() < 2:
            endrun("SurrogateBank.members_apply: five fields of one shape (nz, ..., nens) expected")
        nens = int(fields5[0].shape[-1])
        n = fields5[0].numel() // nens
        if int(nz) < 1 or n % int(nz) != 0:
            endrun("SurrogateBank.members_apply: %d cells per member are not a whole number of columns of nz = %d" % (n, nz))
        if any(t.device != self.device for t in fields5):
            endrun("SurrogateBank.members_apply: the bank lives on %s, the fields on %s" % (self.device, sorted({str(t.device) for t in fields5})))
        check(capi.lib().mw_mlp_set_strict(int(bool(self.strict))))
        with torch.cuda.device(self.device):
            rc = capi.lib().mw_surrogate_members_apply(self._h, (C.c_int * len(members))(*members), int(nz), n // int(nz), nens,
                                                       _field_ptr_array(fields5), _stream_ptr(self.device))
        check(capi.lib().mw_mlp_set_strict(0))
        check(rc)

    def committee_apply(self, nz, sel, member, in5, out4, range4=None):
        """mw_surrogate_committee_apply: the mean of the bank's models sel (1 .. 16 distinct indices, summed in that order) on ensemble
        member `member` of the member-fastest fields in5 = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), each
        (nz, ..., nens), written to out4 = (temp, water_vapor, cloud_liquid, precip_liquid) of the same shape -- each the matching input
        tensor (in place) or a tensor of its own -- and, with range4, the members' largest minus smallest value per cell and field.  Only
        elements of `member` are read and written (self.strict = 1: the thread-per-column form)."""
        sel = [int(s) for s in sel]
        if len(in5) != 5 or len(out4) != 4 or (range4 is not None and len(range4) != 4):
            endrun("SurrogateBank.committee_apply: five input fields, four output fields and (optionally) four range fields expected")
        every = list(in5) + list(out4) + (list(range4) if range4 is not None else [])
        if any(t.shape != in5[0].shape for t in every) or in5[0].dim() < 2:
            endrun("SurrogateBank.committee_apply: fields of one shape (nz, ..., nens) expected")
        if any(t.dtype != torch.float64 or not t.is_contiguous() for t in every):
            endrun("SurrogateBank.committee_apply: contiguous float64 fields expected")
        nens = int(in5[0].shape[-1])
        n = in5[0].numel() // nens
        if int(nz) < 1 or n % int(nz) != 0:
            endrun("SurrogateBank.committee_apply: %d cells per member are not a whole number of columns of nz = %d" % (n, nz))
        if any(t.device != self.device for t in every):
            endrun("SurrogateBank.committee_apply: the bank lives on %s, the fields on %s" % (self.device, sorted({str(t.device) for t in every})))
        check(capi.lib().mw_mlp_set_strict(int(bool(self.strict))))
        with torch.cuda.device(self.device):
            rc = capi.lib().mw_surrogate_committee_apply(self._h, len(sel), (C.c_int * max(1, len(sel)))(*sel), int(member), int(nz), n // int(nz), nens,
                                                         _field_ptr_array(in5), _field_ptr_array(out4),
                                                         _field_ptr_array(range4) if range4 is not None else None, _stream_ptr(self.device))
        check(capi.lib().mw_mlp_set_strict(0))
        check(rc)


def json_safe(x):
    """Nested lists of floats with inf / NaN as the strings "inf", "-inf", "nan" (bare tokens are no JSON); finite numbers unchanged."""
    if isinstance(x, list):
        return [json_safe(v) for v in x]
    return x if np.isfinite(x) else str(float(x))


def _exact_sum_units(x):
    n, d = float(x).as_integer_ratio()
    return n * (_EXACT_ONE // d)


def surrogate_scores(stats, counts):
    """One raw result of SurrogateBank.evaluate as the accumulating form SurrogateEvaluator.combine adds: `sums` (K + 1, 2, 4, 3) exact
    integers in units of 2^-1074, `nonfinite` the same shape in fp64 (a sum that is inf or NaN -- a diverged model -- lives here and its
    integer is 0), `max` (K + 1, 2, 4), `counts` (2,) and the number of calls."""
    stats = np.asarray(stats, dtype=np.float64)
    s = stats[..., :3]
    fin = np.isfinite(s)
    sums = np.zeros(s.shape, dtype=object)
    flat, ff, src = sums.reshape(-1), fin.reshape(-1), s.reshape(-1)
    for i in range(flat.size):
        flat[i] = _exact_sum_units(src[i]) if ff[i] else 0
    return {"sums": sums, "nonfinite": np.where(fin, 0.0, s), "max": stats[..., 3].copy(), "counts": np.asarray(counts, dtype=np.int64).copy(), "calls": 1}


def _sums_to_float(sums, nonfinite):
    out = np.array([v / _EXACT_ONE for v in sums.reshape(-1)], dtype=np.float64).reshape(sums.shape)      # int / int: correctly rounded
    return np.where(nonfinite != 0.0, nonfinite, out)


class SurrogateEvaluator:
    """Scores every model of several banks (one per width) against the microphysics in charge, call after call: accumulate(inp, out) with
    the coupler cloned before micro.time_step and the stepped one (the pair gather_micro_statistics takes), report() at the end.
    names: the models' names, bank after bank."""

    def __init__(self, banks, names):
        self.banks = list(banks)
        self.names = [str(n) for n in names]
        if len(self.names) != sum(b.models for b in self.banks):
            endrun("SurrogateEvaluator: %d names for %d models" % (len(self.names), sum(b.models for b in self.banks)))
        if len(set(self.names)) != len(self.names):
            endrun("SurrogateEvaluator: model names must be unique")
        self.total = None
        self.history = []               # per call: the raw statistics and counts of every bank

    @staticmethod
    def combine(a, b):
        """Two results (lists with one surrogate_scores dict per bank) as one: sums add, maxima take the larger, counts and calls add.  The
        sums are exact integers, so the order of combination cannot matter: (a + b) + c == a + (b + c), also across ranks; by convention
        `a` is the earlier result."""
        if len(a) != len(b):
            endrun("SurrogateEvaluator.combine: results of different evaluators")
        out = []
        for x, y in zip(a, b):
            if x["sums"].shape != y["sums"].shape:
                endrun("SurrogateEvaluator.combine: results of different banks")
            out.append({"sums": x["sums"] + y["sums"], "nonfinite": x["nonfinite"] + y["nonfinite"], "max": np.maximum(x["max"], y["max"]),
                        "counts": x["counts"] + y["counts"], "calls": x["calls"] + y["calls"]})
        return out

    def accumulate(self, inp, out):
        """Runs every bank on (inp, out) and adds the call to the running total; returns the call's own result."""
        names5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
        in5 = [inp.get_data_manager_readonly().get(n, True) for n in names5]
        truth4 = [out.get_data_manager_readonly().get(n, True) for n in EVAL_FIELDS]
        raw = [bank.evaluate(inp.get_nz(), in5, truth4) for bank in self.banks]
        self.history.append([{"stats": json_safe(s.tolist()), "counts": c.tolist()} for s, c in raw])
        one = [surrogate_scores(s, c) for s, c in raw]
        self.total = one if self.total is None else self.combine(self.total, one)
        return one

    def report(self, result=None):
        """Per model (and `persistence:<bank>`), per class (inactive, active, all) and field: n, bias = sum d / n, mae, rmse, max_abs and
        rmse_over_persistence (the skill's denominator: the same class and field of the bank's persistence row).  An empty class has n = 0
        and None for every statistic; so has a ratio whose persistence rmse is 0.  A statistic that is inf or NaN (a diverged model: NaN reaches
        the sums AND max_abs) is None too, and its field carries "finite": False."""
        result = self.total if result is None else result
        if result is None:
            endrun("SurrogateEvaluator.report: nothing accumulated")
        rep, first = {}, 0
        for ib, (bank, r) in enumerate(zip(self.banks, result)):
            sums, nonf = r["sums"], r["nonfinite"]
            # class axis -> (inactive, active, all)
            s3 = _sums_to_float(np.concatenate([sums, sums.sum(axis=1, keepdims=True)], axis=1),
                                np.concatenate([nonf, nonf.sum(axis=1, keepdims=True)], axis=1))
            mx = np.concatenate([r["max"], r["max"].max(axis=1, keepdims=True)], axis=1)
            n = np.concatenate([r["counts"], [r["counts"].sum()]]).astype(np.float64)
            some = n > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                per = s3 / np.where(some, n, 1.0)[None, :, None, None]
                rmse = np.sqrt(per[..., 2])
                skill = rmse / rmse[-1:]
            ok_skill = some[None, :, None] & (rmse[-1:] > 0)
            for m in range(bank.models + 1):
                name = self.names[first + m] if m < bank.models else "persistence:%d" % ib
                rep[name] = {}
                for c, cname in enumerate(EVAL_CLASSES + ("all",)):
                    row = {"n": int(n[c])}
                    for v, fname in enumerate(EVAL_FIELDS):
                        if some[c]:
                            row[fname] = {"bias": float(per[m, c, v, 0]), "mae": float(per[m, c, v, 1]), "rmse": float(rmse[m, c, v]),
                                          "max_abs": float(mx[m, c, v]),
                                          "rmse_over_persistence": float(skill[m, c, v]) if ok_skill[0, c, v] else None}
                            if not all(x is None or np.isfinite(x) for x in row[fname].values()):
                                row[fname] = {k: (x if x is not None and np.isfinite(x) else None) for k, x in row[fname].items()}
                                row[fname]["finite"] = False
                        else:
                            row[fname] = {"bias": None, "mae": None, "rmse": None, "max_abs": None, "rmse_over_persistence": None}
                    rep[name][cname] = row
            first += bank.models
        return rep

    def table(self, rep=None):
        """report() as text: one line per model and class, rmse / persistence rmse per field (the skill: < 1 beats doing nothing)."""
        rep = self.report() if rep is None else rep
        w = max(len(k) for k in rep)
        lines = ["%-*s %-8s %12s " % (w, "model", "class", "n") + " ".join("%26s" % ("%s rmse (/pers.)" % f) for f in EVAL_FIELDS)]
        for name, classes in rep.items():
            for cname, row in classes.items():
                cells = []
                for f in EVAL_FIELDS:
                    r, q = row[f]["rmse"], row[f]["rmse_over_persistence"]
                    cells.append("%26s" % ("-" if r is None else "%.6e (%s)" % (r, "-" if q is None else "%.4g" % q)))
                lines.append("%-*s %-8s %12d " % (w, name, cname, row["n"]) + " ".join(cells))
        return "\n".join(lines)


class _CommitteeRow:
    models = 1            # what SurrogateEvaluator.report reads of a bank: the committee is the one "model" beside the persistence row


def committee_score(nz, in5, truth4, pred4, range4, workspace=None):
    """mw_committee_score on contiguous fp64 CUDA fields of nz levels: returns (stats (2, 4, 7) fp64 = [class][field][sum d, sum |d|,
    sum d^2, max |d|, sum r, sum r^2, sum r |d|], counts (2,) int64 cells per class, covered (2, 4) int64 cells with |d| <= r), d = pred -
    truth, r = range; classes as SurrogateBank.evaluate -- one device-to-host copy."""
    every = list(in5) + list(truth4) + list(pred4) + list(range4)
    if (len(in5), len(truth4), len(pred4), len(range4)) != (5, 4, 4, 4):
        endrun("committee_score: five input fields and four truth, prediction and range fields expected")
    n, dev = in5[0].numel(), in5[0].device
    if int(nz) < 1 or n % int(nz) != 0 or any(t.numel() != n for t in every):
        endrun("committee_score: the seventeen fields must have one size, a whole number of columns of nz = %d levels" % nz)
    if any(t.device != dev or t.dtype != torch.float64 or not t.is_contiguous() for t in every):
        endrun("committee_score: contiguous float64 fields of one device expected")
    L = capi.lib()
    nbytes = L.mw_committee_score_workspace_bytes(int(nz), n // int(nz))
    if workspace is None or workspace.numel() * 8 < nbytes:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    buf = torch.empty(56 + 10, dtype=torch.int64, device=dev)                   # the statistics' bytes, then the ten counts
    with torch.cuda.device(dev):
        check(L.mw_committee_score(int(nz), n // int(nz), _field_ptr_array(in5), _field_ptr_array(truth4), _field_ptr_array(pred4),
                                   _field_ptr_array(range4), _ptr(workspace), C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 8 * 56),
                                   _stream_ptr(dev)))
    host = buf.cpu().numpy()
    return host[:56].view(np.float64).reshape(2, 4, 7).copy(), host[56:58].copy(), host[58:].reshape(2, 4).copy()


def _exact_units_array(x):
    """(exact integers in units of 2^-1074, the non-finite values apart) of an fp64 array: surrogate_scores' split."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    units = np.zeros(x.shape, dtype=object)
    flat, ff, src = units.reshape(-1), fin.reshape(-1), x.reshape(-1)
    for i in range(flat.size):
        flat[i] = _exact_sum_units(src[i]) if ff[i] else 0
    return units, np.where(fin, 0.0, x)


def range_error_correlation(n, sum_r, sum_r2, sum_a, sum_a2, sum_ra):
    """Pearson's r of the range r and the error |d| over n cells from their six sums; None when a sum is not finite or a variance is not
    positive (a constant range, a perfect prediction, an empty class)."""
    vals = (sum_r, sum_r2, sum_a, sum_a2, sum_ra)
    if n < 1 or not all(np.isfinite(v) for v in vals):
        return None
    mr, ma = sum_r / n, sum_a / n
    vr, va = sum_r2 / n - mr * mr, sum_a2 / n - ma * ma
    if not (vr > 0.0 and va > 0.0):
        return None
    q = (sum_ra / n - mr * ma) / np.sqrt(vr * va)
    return float(min(1.0, max(-1.0, q))) if np.isfinite(q) else None


class CommitteeEvaluator:
    """Scores the committee `sel` of a bank against the microphysics in charge, call after call, as SurrogateEvaluator scores single
    models: accumulate(inp, out) runs the committee forward into scratch fields (mean and range) and mw_committee_score on them, report()
    gives per class (inactive, active, all) and field the evaluator's row (bias, mae, rmse, max_abs, rmse_over_persistence) plus mean_range,
    coverage (the fraction of cells with |d| <= range) and range_error_correlation (range_error_correlation above)."""

    def __init__(self, bank, sel):
        self.bank, self.sel = bank, [int(i) for i in sel]
        if not 1 <= len(self.sel) <= capi.MW_COMMITTEE_MAX_MODELS:
            endrun("CommitteeEvaluator: a committee has 1 to %d models, got %d" % (capi.MW_COMMITTEE_MAX_MODELS, len(self.sel)))
        if len(set(self.sel)) != len(self.sel) or any(not 0 <= i < bank.models for i in self.sel):
            endrun("CommitteeEvaluator: the committee must name distinct models of the bank's %d" % bank.models)
        self.total = None
        self.history = []
        self._scratch = None
        self._ws = None

    def accumulate(self, inp, out):
        """One call: the committee's mean and range from `inp`, scored against `out`; added to the running total.  Returns the call's raw
        (stats (2, 2, 4, 7) = [committee | persistence], counts (2,), covered (2, 4))."""
        names5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
        nz = inp.get_nz()
        in5 = [inp.get_data_manager_readonly().get(n, True) for n in names5]
        truth4 = [out.get_data_manager_readonly().get(n, True) for n in EVAL_FIELDS]
        if self._scratch is None or self._scratch[0].shape != in5[0].shape:
            self._scratch = [torch.empty_like(in5[0]) for _ in range(8)]
        pred4, range4 = self._scratch[:4], self._scratch[4:]
        as1 = lambda ts: [t.reshape(nz, -1, 1) for t in ts]                     # noqa: E731   (every member is one more column)
        self.bank.committee_apply(nz, self.sel, 0, as1(in5), as1(pred4), as1(range4))
        if self._ws is None:
            self._ws = torch.empty((capi.lib().mw_committee_score_workspace_bytes(nz, in5[0].numel() // nz) + 7) // 8, dtype=torch.float64,
                                   device=in5[0].device)
        stats, counts, covered = committee_score(nz, in5, truth4, pred4, range4, self._ws)
        pstats, _, _ = committee_score(nz, in5, truth4, [in5[0], in5[2], in5[3], in5[4]], range4, self._ws)      # persistence: prediction = input
        both = np.stack([stats, pstats])
        self.history.append({"stats": json_safe(both.tolist()), "counts": counts.tolist(), "covered": covered.tolist()})
        units, nonf = _exact_units_array(stats[..., 4:])
        one = {"scores": [surrogate_scores(both[..., :4], counts)], "rsums": units, "rnonfinite": nonf, "covered": covered.astype(np.int64)}
        if self.total is None:
            self.total = one
        else:
            t = self.total
            self.total = {"scores": SurrogateEvaluator.combine(t["scores"], one["scores"]), "rsums": t["rsums"] + units,
                          "rnonfinite": t["rnonfinite"] + nonf, "covered": t["covered"] + one["covered"]}
        return both, counts, covered

    def report(self):
        if self.total is None:
            endrun("CommitteeEvaluator.report: nothing accumulated")
        t = self.total
        base = SurrogateEvaluator([_CommitteeRow()], ["committee"]).report(t["scores"])["committee"]
        sc = t["scores"][0]
        counts = np.concatenate([sc["counts"], [sc["counts"].sum()]])
        with3 = lambda a: np.concatenate([a, a.sum(axis=0, keepdims=True)], axis=0)      # noqa: E731   class axis -> (inactive, active, all)
        rs = _sums_to_float(with3(t["rsums"]), with3(t["rnonfinite"]))                 # (3, 4, 3): sum r, sum r^2, sum r |d|
        ds = _sums_to_float(with3(sc["sums"][0]), with3(sc["nonfinite"][0]))           # (3, 4, 3): sum d, sum |d|, sum d^2
        cov = with3(t["covered"])
        rep = {}
        for c, cname in enumerate(EVAL_CLASSES + ("all",)):
            n = int(counts[c])
            row = {"n": n}
            for v, fname in enumerate(EVAL_FIELDS):
                f = dict(base[cname][fname])
                if n > 0:
                    mr = rs[c, v, 0] / n
                    f["mean_range"] = float(mr) if np.isfinite(mr) else None
                    f["coverage"] = int(cov[c, v]) / n
                    f["range_error_correlation"] = range_error_correlation(n, rs[c, v, 0], rs[c, v, 1], ds[c, v, 1], ds[c, v, 2], rs[c, v, 2])
                    if f["mean_range"] is None:
                        f["finite"] = False
                else:
                    f.update(mean_range=None, coverage=None, range_error_correlation=None)
                row[fname] = f
            rep[cname] = row
        return rep

    def table(self, rep=None, name="committee"):
        """report() as text: one line per class; rmse / persistence rmse, mean range and coverage per field."""
        rep = self.report() if rep is None else rep
        lines = ["%-16s %-8s %12s " % ("committee", "class", "n") + " ".join("%40s" % ("%s rmse (/pers.) range cover" % f) for f in EVAL_FIELDS)]
        fmt = lambda x, p: "-" if x is None else p % x                                # noqa: E731
        for cname, row in rep.items():
            cells = ["%40s" % ("%s (%s) %s %s" % (fmt(row[f]["rmse"], "%.4e"), fmt(row[f]["rmse_over_persistence"], "%.4g"),
                                                   fmt(row[f]["mean_range"], "%.3e"), fmt(row[f]["coverage"], "%.3f"))) for f in EVAL_FIELDS]
            lines.append("%-16s %-8s %12d " % (name, cname, row["n"]) + " ".join(cells))
        return "\n".join(lines)


# ---- candidate surrogates rolled out as ensemble members beside Kessler ----------------------------------------------------------------
ROLLOUT_FIELDS = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor", "cloud_liquid", "precip_liquid")
ROLLOUT_STATS = ("sum_d", "sum_abs_d", "sum_d2", "max_abs_d", "sum_x", "min_x", "max_x")
ROLLOUT_WATER = ("water_vapor", "cloud_liquid", "precip_liquid")
ROLLOUT_IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")     # fields5 of members_apply and of the teacher


def rollout_member_names(model_names, persistence=True, committees=()):
    """The fixed roles of a rollout's ensemble members: member 0 is Kessler, members 1 .. K the models of the list in its order, then one
    member per committee (names of `committees`, in its order), an optional last member persistence (no microphysics).  More members than
    the dycore steps in one call is an error that names the limit."""
    names = [str(n) for n in model_names]
    if len(set(names)) != len(names) or {"kessler", "persistence"} & set(names):
        endrun("rollout: model names must be unique and neither 'kessler' nor 'persistence'")
    cnames = [str(n) for n in committees]
    if len(set(cnames)) != len(cnames) or ({"kessler", "persistence"} | set(names)) & set(cnames):
        endrun("rollout: committee names must be unique and neither a model's name nor 'kessler' nor 'persistence'")
    members = ["kessler"] + names + cnames + (["persistence"] if persistence else [])
    if len(members) > capi.MW_ROLLOUT_MAX_MEMBERS:
        endrun("rollout: %d models%s%s beside Kessler are %d ensemble members, the dycore steps at most %d"
               % (len(names), (", %d committees" % len(cnames)) if cnames else "", " and persistence" if persistence else "", len(members),
                  capi.MW_ROLLOUT_MAX_MEMBERS))
    return members


class Microphysics_Rollout(Microphysics_Kessler):
    """One microphysics step that treats every ensemble member differently (no reference counterpart): member 0 is stepped by Kessler,
    member k by model k - 1 of `models` (its output written back: Microphysics_Kessler_Surrogate.online for that member), the optional last
    member by nothing.  The dycore, the sponge and the nudger step the members independently, so one run shows how each candidate behaves
    once its own output is fed back.  Kessler runs on member 0 ALONE, extracted to contiguous arrays: its rain sub-cycle count is a minimum
    over all the columns of a call.  `precl` is written for member 0 only; the other members' precl keeps whatever it held.
    With a `harvester` (RolloutHarvester) and `harvest_now` set, the step harvests Kessler labels on the model members' own states
    between the Kessler member's step and the models'; harvesting reads the state and never writes it."""

    mlp_strict = 0        # 1: the thread-per-cell MLP kernels (mw_mlp_set_strict)
    harvester = None      # a RolloutHarvester: time_step harvests when harvest_now is set (the driver sets it, and harvest_etime, per step)
    harvest_now = False
    harvest_etime = 0.0

    def micro_name(self):
        return "rollout"

    def init(self, coupler, models, persistence=True, names=None, committees=()):
        """models: (W1, b1, W2, b2, scl_in, scl_out) tuples as load_surrogate_weights returns them, single-cell and stencil networks in any
        order; names: theirs (default model0, model1, ...).  committees: (name, [model names]) pairs; each is one more member after the
        models, replaced in place from its OWN state by the mean of its models (1 .. 16 of one width, SurrogateBank.committee_apply on that
        width's bank).  The coupler must have 1 + len(models) + len(committees) (+ 1 with persistence) members."""
        models = list(models)
        names = ["model%d" % k for k in range(len(models))] if names is None else [str(n) for n in names]
        if len(names) != len(models):
            endrun("Microphysics_Rollout: %d names for %d models" % (len(names), len(models)))
        committees = [(str(c[0]), [str(n) for n in c[1]]) for c in committees]
        self.member_names = rollout_member_names(names, persistence, [c[0] for c in committees])
        self.persistence = bool(persistence)
        if coupler.get_nens() != len(self.member_names):
            endrun("Microphysics_Rollout: %d models%s%s beside Kessler need nens = %d, the coupler has %d"
                   % (len(models), (", %d committees" % len(committees)) if committees else "", " and persistence" if persistence else "",
                      len(self.member_names), coupler.get_nens()))
        for cname, cmodels in committees:
            if not 1 <= len(cmodels) <= capi.MW_COMMITTEE_MAX_MODELS:
                endrun("Microphysics_Rollout: committee %r has %d models, a committee has 1 to %d" % (cname, len(cmodels), capi.MW_COMMITTEE_MAX_MODELS))
            if len(set(cmodels)) != len(cmodels) or any(n not in names for n in cmodels):
                endrun("Microphysics_Rollout: committee %r must name distinct models of the list (%s)" % (cname, ", ".join(names)))
            if len({int(np.shape(models[names.index(n)][0])[0]) for n in cmodels}) != 1:
                endrun("Microphysics_Rollout: committee %r mixes single-cell and stencil models: a committee has one width" % cname)
        super().init(coupler)
        coupler.set_option("micro", "rollout")
        widths = []
        for m in models:
            if int(np.shape(m[0])[0]) not in widths:
                widths.append(int(np.shape(m[0])[0]))
        # one bank per width; a model keeps the member its place in the list gives it
        self.banks = [(SurrogateBank([m for m in models if np.shape(m[0])[0] == w], coupler.device),
                       [1 + k for k, m in enumerate(models) if np.shape(m[0])[0] == w]) for w in widths]
        # a committee runs on its width's bank: (bank, its models' places in that bank, its member)
        self.committees = []
        for ci, (cname, cmodels) in enumerate(committees):
            w = int(np.shape(models[names.index(cmodels[0])][0])[0])
            in_bank = [k for k, m in enumerate(models) if np.shape(m[0])[0] == w]
            self.committees.append((self.banks[widths.index(w)][0], [in_bank.index(names.index(n)) for n in cmodels], 1 + len(models) + ci))
        self._m0 = None

    def time_step(self, coupler, dt):
        dm = coupler.get_data_manager_readwrite()
        temp, rho_d = dm.get("temp"), dm.get("density_dry", readonly=True)
        rho_v, rho_c, rho_r, precl = dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid"), dm.get("precl")
        nz, nens = coupler.get_nz(), coupler.get_nens()
        ncol = coupler.get_ny() * coupler.get_nx()
        n = nz * ncol
        L = capi.lib()
        if self._m0 is None or self._m0[0][0].numel() != n or self._m0[1].numel() != ncol:
            self._m0 = ([torch.empty(n, dtype=torch.float64, device=coupler.device) for _ in range(5)],
                        torch.empty(ncol, dtype=torch.float64, device=coupler.device))
        (v0, c0, r0, d0, t0), p0 = self._m0
        nbytes = L.mw_kessler_workspace_bytes(nz, ncol)
        if self._ws is None or self._ws.numel() * 8 < nbytes:
            self._ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=coupler.device)
        st = _stream_ptr(coupler.device)
        check(L.mw_kessler_set_strict(self.strict))
        with torch.cuda.device(coupler.device):
            check(L.mw_member_extract(n, nens, 0, 5, _field_ptr_array([rho_v, rho_c, rho_r, rho_d, temp]), _field_ptr_array([v0, c0, r0, d0, t0]), st))
            check(L.mw_kessler_time_step(nz, ncol, coupler.get_dz(), float(dt), _ptr(v0), _ptr(c0), _ptr(r0), _ptr(d0), _ptr(t0), _ptr(p0),
                                         _ptr(self._ws), None, st))
            check(L.mw_member_insert(n, nens, 0, 4, _field_ptr_array([v0, c0, r0, t0]), _field_ptr_array([rho_v, rho_c, rho_r, temp]), st))
            check(L.mw_member_insert(ncol, nens, 0, 1, _field_ptr_array([p0]), _field_ptr_array([precl]), st))
        if self.harvester is not None and self.harvest_now:                    # the teacher sees the state each model is about to replace
            self.last_harvest = self.harvester.harvest(coupler, dt, self.harvest_etime)
        for bank, members in self.banks:
            bank.strict = self.mlp_strict
            bank.members_apply(nz, members, [temp, rho_d, rho_v, rho_c, rho_r])
        for bank, sel, member in getattr(self, "committees", ()):
            bank.strict = self.mlp_strict
            bank.committee_apply(nz, sel, member, [temp, rho_d, rho_v, rho_c, rho_r], [temp, rho_v, rho_c, rho_r])


def kessler_members_teacher(coupler, members, dt, max_rainsplit=64, outs=None, return_rainsplit=False):
    """mw_kessler_members_teacher on the coupler's member-fastest fields: what Kessler would do to the state of every member in `members`,
    each member alone, out of place.  Returns the four teacher tensors (temp, water_vapor, cloud_liquid, precip_liquid after Kessler), each
    (nz, ny, nx, nens); only the listed members' elements are written (outs: four tensors to write into, default new uninitialised ones).
    A member whose own state asks for more than max_rainsplit rain sub-cycles, or whose rain CFL step is not a positive finite number, is
    skipped: not computed, not written.  return_rainsplit=True: (tensors, counts per listed member, 0 = skipped), at the price of a
    stream synchronisation.  The coupler's fields are read only."""
    dm = coupler.get_data_manager_readonly()
    f5 = [dm.get(n, True) for n in ROLLOUT_IN5]
    members = [int(m) for m in members]
    nz, nens = coupler.get_nz(), coupler.get_nens()
    ncol = coupler.get_ny() * coupler.get_nx()
    if outs is None:
        outs = [torch.empty_like(f5[0]) for _ in range(4)]
    if len(outs) != 4 or any(o.shape != f5[0].shape or o.device != f5[0].device for o in outs):
        endrun("kessler_members_teacher: outs must be four tensors of the fields' shape on their device")
    L = capi.lib()
    nbytes = L.mw_kessler_members_teacher_workspace_bytes(nz, ncol, nens)
    if nbytes <= 0:
        endrun("kessler_members_teacher: nz = %d, %d columns and %d members are out of range (nz >= 2, at most 64 members)" % (nz, ncol, nens))
    ws = getattr(coupler, "_ws_teacher", None)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = coupler._ws_teacher = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=coupler.device)
    rs = (C.c_int * max(1, len(members)))()
    with torch.cuda.device(coupler.device):
        check(L.mw_kessler_members_teacher(nz, ncol, nens, len(members), (C.c_int * max(1, len(members)))(*members), coupler.get_dz(), float(dt),
                                           int(max_rainsplit), _field_ptr_array(f5), _field_ptr_array(outs), rs if return_rainsplit else None,
                                           _ptr(ws), _stream_ptr(coupler.device)))
    return (outs, [int(rs[j]) for j in range(len(members))]) if return_rainsplit else outs


class RolloutHarvester:
    """Data aggregation for the rollout (no reference counterpart): while the candidate models run online as ensemble members, ask the
    teacher -- Kessler -- what it would have done to each model member's OWN state, and keep (state, label) samples of it in one file per
    member, `rollout_samples_<name>.nc`, with exactly DataGenerator's dimensions and variables (surrogate_train.read_samples takes them
    unchanged).  harvest() is teacher -> mask -> nonzero -> gather -> append; the coupler's state is read, never written."""

    def init(self, coupler, member_names, members, directory, samples_per_step=50, ratio_active=0.5, prior_active=0.4, seed=None,
             max_rainsplit=64):
        """member_names / members: the harvested model members' names and ensemble indices.  samples_per_step, ratio_active: the wanted
        samples per call and member and the wanted share of active cells among them (DataGenerator's 50 and 0.5); prior_active: the share
        of active cells assumed when the thresholds are set (DataGenerator's 0.4); seed: call c draws with seed + c (default: the clock)."""
        import time as _time
        self.member_names, self.members = [str(n) for n in member_names], [int(m) for m in members]
        if len(self.member_names) != len(self.members) or not self.members or len(set(self.members)) != len(self.members) or \
                len(set(self.member_names)) != len(self.members):
            endrun("RolloutHarvester: as many distinct names as distinct members, at least one")
        if any(not 0 <= m < coupler.get_nens() for m in self.members):
            endrun("RolloutHarvester: members %r outside [0, %d)" % (self.members, coupler.get_nens()))
        if not (samples_per_step > 0 and 0.0 < ratio_active < 1.0 and 0.0 < prior_active < 1.0 and 1 <= int(max_rainsplit) <= 1024):
            endrun("RolloutHarvester: samples_per_step > 0, ratio_active and prior_active in (0, 1), max_rainsplit in [1, 1024]")
        self.samples_per_step, self.ratio_active, self.prior_active = float(samples_per_step), float(ratio_active), float(prior_active)
        self.max_rainsplit = int(max_rainsplit)
        self.seed = int(_time.time()) if seed is None else int(seed)
        self.files = {n: os.path.join(directory, "rollout_samples_%s.nc" % n) for n in self.member_names}
        for f in self.files.values():
            _sample_file_create(f)
        self.samples = {n: 0 for n in self.member_names}
        self.skipped = {n: 0 for n in self.member_names}
        self.calls = 0
        self._meta_written = False
        self._teacher = None
        self.last_elems = None

    def thresholds(self, coupler):
        """DataGenerator's two formulas (generate_micro_surrogate_data.h:58-62) per member, clamped to 1."""
        ncell = coupler.get_nz() * coupler.get_ny() * coupler.get_nx()
        thr_act = self.ratio_active * self.samples_per_step / (self.prior_active * ncell)
        thr_inact = (1 - self.ratio_active) * self.samples_per_step / ((1 - self.prior_active) * ncell)
        return min(1.0, thr_act), min(1.0, thr_inact)

    def harvest(self, coupler, dt, etime):
        """One call: {name: samples added}.  A member the teacher skipped adds none and counts in `skipped`."""
        dm = coupler.get_data_manager_readonly()
        f5 = [dm.get(n, True) for n in ROLLOUT_IN5]
        nz, nens = coupler.get_nz(), coupler.get_nens()
        ncol = coupler.get_ny() * coupler.get_nx()
        nelem = nz * ncol * nens
        dev = coupler.device
        if self._teacher is None or self._teacher[0].shape != f5[0].shape:
            self._teacher = [torch.empty_like(f5[0]) for _ in range(4)]
        teacher, rs = kessler_members_teacher(coupler, self.members, dt, self.max_rainsplit, self._teacher, return_rainsplit=True)
        live = [(n, m) for n, m, r in zip(self.member_names, self.members, rs) if r > 0]
        for n, r in zip(self.member_names, rs):
            self.skipped[n] += int(r == 0)
        thr_act, thr_inact = self.thresholds(coupler)
        max_mag = (2 ** 64 - 1) // (1 + nelem)
        key0 = (((self.seed + self.calls) % max_mag) * nelem) % (2 ** 64)
        self.calls += 1
        added = {n: 0 for n in self.member_names}
        write_meta, self._meta_written = not self._meta_written, True
        ins = outs = which = None
        if live:
            L = capi.lib()
            mask = torch.empty(nelem, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                check(L.mw_member_sample_mask(nz, ncol, nens, len(live), (C.c_int * len(live))(*[m for _, m in live]), _field_ptr_array(f5),
                                              _field_ptr_array(teacher), key0, thr_act, thr_inact, C.c_void_p(mask.data_ptr()), _stream_ptr(dev)))
                elems = torch.nonzero(mask).flatten().contiguous()             # ascending, as DataGenerator compacts
                n = int(elems.numel())
                ins = torch.empty((n, 5, 2), dtype=torch.float32, device=dev)
                outs = torch.empty((n, 4), dtype=torch.float32, device=dev)
                check(L.mw_member_gather_samples(nz, ncol, nens, _field_ptr_array(f5), _field_ptr_array(teacher), C.c_void_p(elems.data_ptr()), n,
                                                 C.c_void_p(ins.data_ptr()), C.c_void_p(outs.data_ptr()), _stream_ptr(dev)))
            self.last_elems = elems.cpu().numpy()                              # (k * ncol + col) * nens + member of the samples (diagnostic)
            ins, outs, which = ins.cpu().numpy(), outs.cpu().numpy(), self.last_elems % nens
        else:
            self.last_elems = np.zeros(0, dtype=np.int64)
        for name, m in zip(self.member_names, self.members):
            sel = (which == m) if which is not None else np.zeros(0, dtype=bool)
            a = ins[sel] if which is not None else np.zeros((0, 5, 2), dtype=np.float32)
            b = outs[sel] if which is not None else np.zeros((0, 4), dtype=np.float32)
            _sample_file_append(self.files[name], coupler, dt, a, b, write_meta)
            added[name] = int(a.shape[0])
            self.samples[name] += added[name]
        return added


def member_divergence(coupler, names):
    """mw_member_divergence of the coupler's fields `names` (at most 16, each (..., nens)): the raw arrays (stats, nonfinite) --
    stats (nens, len(names), 7) fp64 in the order of ROLLOUT_STATS (d = member - member 0 for the first four, the member's own values for
    the last three), nonfinite (nens, len(names)) int64, the member's NaN or inf elements -- from one device-to-host copy."""
    dm = coupler.get_data_manager_readonly()
    fields = [dm.get(n, True) for n in names]
    nens = coupler.get_nens()
    n = fields[0].numel() // nens
    if any(t.numel() != n * nens or t.shape[-1] != nens for t in fields):
        endrun("member_divergence: the fields must have one size and the members last")
    L = capi.lib()
    nf = len(fields)
    nbytes = L.mw_member_divergence_workspace_bytes(n, nens, nf)
    if nbytes <= 0:
        endrun("member_divergence: %d fields of %d cells x %d members are out of range (at most %d fields)" % (nf, n, nens, capi.MW_MAX_TRACERS))
    ws = getattr(coupler, "_ws_divergence", None)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = coupler._ws_divergence = torch.empty(nbytes // 8, dtype=torch.float64, device=coupler.device)
    buf = torch.empty(nens * nf * 8, dtype=torch.int64, device=coupler.device)             # the statistics' bytes, then the counts
    nout = nens * nf * 7
    with torch.cuda.device(coupler.device):
        check(L.mw_member_divergence(n, nens, nf, _field_ptr_array(fields), _ptr(ws), C.c_void_p(buf.data_ptr()),
                                     C.c_void_p(buf.data_ptr() + 8 * nout), _stream_ptr(coupler.device)))
    host = buf.cpu().numpy()
    return host[:nout].view(np.float64).reshape(nens, nf, 7).copy(), host[nout:].reshape(nens, nf).copy()


def rollout_report(stats, nonfinite, ncells, member_names, fields, cell_volume=1.0, persistence=None):
    """One scoring time's raw arrays (member_divergence) as a report -- pure numpy.  Per member and field: bias = sum d / n, mae, rmse and
    max_abs of d = member - Kessler member, rmse_over_persistence (None without a persistence member `persistence`, or when its rmse is
    0), the member's own mean, min, max and its count of non-finite elements.  A statistic that is inf or NaN is None and the field
    carries "finite": False.  Per member: total_water = cell_volume * sum of the three water fields (None unless all three are scored
    and finite) and finite = no field has a non-finite element or statistic."""
    stats = np.asarray(stats, dtype=np.float64)
    nonfinite = np.asarray(nonfinite, dtype=np.int64)
    if stats.shape != (len(member_names), len(fields), 7) or nonfinite.shape != stats.shape[:2]:
        endrun("rollout_report: stats must be (%d members, %d fields, 7) and nonfinite (%d, %d)" % ((len(member_names), len(fields)) * 2))
    n = float(ncells)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rmse = np.sqrt(stats[..., 2] / n)
        skill = rmse / rmse[persistence] if persistence is not None else None
    rep = {}
    for m, mname in enumerate(member_names):
        row, ok_member = {}, True
        for f, fname in enumerate(fields):
            q = None
            if persistence is not None and rmse[persistence, f] > 0:
                q = float(skill[m, f])
            cell = {"bias": float(stats[m, f, 0] / n), "mae": float(stats[m, f, 1] / n), "rmse": float(rmse[m, f]), "max_abs": float(stats[m, f, 3]),
                    "rmse_over_persistence": q, "mean": float(stats[m, f, 4] / n), "min": float(stats[m, f, 5]), "max": float(stats[m, f, 6]),
                    "nonfinite": int(nonfinite[m, f])}
            if nonfinite[m, f] != 0 or not all(x is None or np.isfinite(x) for x in cell.values()):
                cell = {k: (x if x is not None and np.isfinite(x) else None) for k, x in cell.items()}
                cell["finite"] = False
                ok_member = False
            row[fname] = cell
        water = None
        if all(w in fields for w in ROLLOUT_WATER):
            water = float(sum(stats[m, list(fields).index(w), 4] for w in ROLLOUT_WATER) * cell_volume)
            water = water if np.isfinite(water) else None
        rep[mname] = {"fields": row, "total_water": water, "finite": ok_member}
    return rep


class RolloutScorer:
    """Online skill of a rollout's members: accumulate(coupler, step, etime) at every scoring time, report() / table() at the end.
    member_names: rollout_member_names' list (a last member called persistence is the skill's denominator); fields: the coupler fields
    to score."""

    def __init__(self, member_names, fields=ROLLOUT_FIELDS):
        self.member_names = [str(m) for m in member_names]
        self.fields = [str(f) for f in fields]
        self.persistence = len(self.member_names) - 1 if self.member_names[-1] == "persistence" else None
        self.history = []               # per scoring time: step, etime, the raw arrays
        self.times = []                 # per scoring time: step, etime, rollout_report
        self.diverged_at = {m: None for m in self.member_names}

    def add(self, stats, nonfinite, ncells, cell_volume, step, etime):
        """One scoring time from raw arrays (what accumulate does after member_divergence): pure numpy."""
        rep = rollout_report(stats, nonfinite, ncells, self.member_names, self.fields, cell_volume, self.persistence)
        self.history.append({"step": int(step), "etime": float(etime), "stats": json_safe(np.asarray(stats, dtype=np.float64).tolist()),
                             "nonfinite": np.asarray(nonfinite).tolist()})
        self.times.append({"step": int(step), "etime": float(etime), "members": rep})
        for m in self.member_names:
            if self.diverged_at[m] is None and not rep[m]["finite"]:
                self.diverged_at[m] = {"step": int(step), "etime": float(etime)}
        return rep

    def accumulate(self, coupler, step, etime):
        stats, nonfinite = member_divergence(coupler, self.fields)
        ncells = coupler.get_nz() * coupler.get_ny() * coupler.get_nx()
        return self.add(stats, nonfinite, ncells, coupler.get_dx() * coupler.get_dy() * coupler.get_dz(), step, etime)

    def report(self):
        """{"times": one rollout_report per scoring time with its step and etime, "diverged_at": per member the first scoring time at
        which it showed a non-finite value, or None}."""
        if not self.times:
            endrun("RolloutScorer.report: nothing accumulated")
        return {"times": self.times, "diverged_at": dict(self.diverged_at)}

    def table(self, rep=None):
        """The last scoring time as text: one line per member, rmse against the Kessler member (/ persistence rmse) per field."""
        rep = self.report() if rep is None else rep
        last = rep["times"][-1]
        w = max(len(m) for m in self.member_names)
        lines = ["step %d, etime %.6f s" % (last["step"], last["etime"]),
                 "%-*s " % (w, "member") + " ".join("%26s" % ("%s rmse (/pers.)" % f) for f in self.fields) + "  diverged_at"]
        for m in self.member_names:
            cells = []
            for f in self.fields:
                r, q = last["members"][m]["fields"][f]["rmse"], last["members"][m]["fields"][f]["rmse_over_persistence"]
                cells.append("%26s" % ("-" if r is None else "%.6e (%s)" % (r, "-" if q is None else "%.4g" % q)))
            d = rep["diverged_at"][m]
            lines.append("%-*s " % (w, m) + " ".join(cells) + "  " + ("-" if d is None else "step %d" % d["step"]))
        return "\n".join(lines)


def perturb_temperature(coupler, thermal=True, random=False):                   # perturb_temperature.h:8-67
    temp = coupler.get_data_manager_readwrite().get("temp")
    with torch.cuda.device(coupler.device):
        if random:      # :25-39 (splitmix64 in place of the unavailable yakl::Random, see include/mw_cdna4.h)
            check(capi.lib().mw_perturb_temperature_random(C.byref(coupler.grid), _ptr(temp), _stream_ptr(coupler.device)))
        if thermal:     # :41-66
            check(capi.lib().mw_perturb_temperature(C.byref(coupler.grid), _ptr(temp), _stream_ptr(coupler.device)))


def use_rccl_allreduce(coupler, dycore):
    """The column modules' sums over ranks (sponge_layer, ColumnNudger) on the dycore handle's own RCCL communicator
    (mw_dycore_rccl_allreduce_sum, ctx = the handle) instead of torch.distributed -- what a C++ host does (host/mw_facade.h)."""
    fn = C.cast(capi.lib().mw_dycore_rccl_allreduce_sum, capi.ALLREDUCE_FN)
    coupler._allreduce = (fn, dycore.h, dycore)


def _torch_allreduce(coupler, group=None):
    """-> (mw_allreduce_fn, ctx) for the sponge / nudger horizontal means: the override installed by use_rccl_allreduce, else
    torch.distributed (RCCL on GPUs); (NULL, None) on one rank."""
    ov = getattr(coupler, "_allreduce", None)
    if ov is not None:
        return ov[0], ov[1]
    import torch.distributed as dist
    if coupler.get_nranks() <= 1 or not dist.is_initialized():
        return C.cast(None, capi.ALLREDUCE_FN), None
    dev = coupler.device

    def cb(ctx, buf, n, stream):
        try:
            class _A:
                pass
            a = _A()
            a.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f8", data=(int(buf), False), version=2)
            st = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
            with torch.cuda.device(dev), torch.cuda.stream(st):
                t = torch.as_tensor(a, device=dev)
                if dist.get_backend(group) == "gloo":
                    h = t.cpu(); dist.all_reduce(h, group=group); t.copy_(h)
                else:
                    dist.all_reduce(t, group=group)
            return 0
        except Exception as e:                                   # pragma: no cover
            import sys
            print("allreduce callback failed: %r" % (e,), file=sys.stderr)
            return 1
    fn = capi.ALLREDUCE_FN(cb)
    coupler._allreduce_keep = fn                                 # (the callback object must outlive the call)
    return fn, None


def _field_ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = _ptr(t).value
    return arr


def _column_ws(coupler, nf, holder):
    nbytes = capi.lib().mw_column_workspace_bytes(C.byref(coupler.grid), nf)
    ws = getattr(holder, "_ws_col", None)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=coupler.device)
        holder._ws_col = ws
    return ws


def set_column_strict(strict):
    """1: sponge_layer / ColumnNudger add their horizontal sums in the reference's serial order (bit-identical to the CPU restatement);
    0: the deterministic tree sums (default).  Process-wide (mw_column_set_strict)."""
    check(capi.lib().mw_column_set_strict(int(bool(strict))))


def sponge_layer(coupler, dt, time_scale=60.0):
    """modules::sponge_layer(coupler, dt, time_scale), model/modules/sponge_layer.h:8-77."""
    dm = coupler.get_data_manager_readwrite()
    fields = [dm.get(n) for n in ("density_dry", "uvel", "vvel", "wvel", "temp")] + [dm.get(n) for n in coupler.get_tracer_names()]
    ws = _column_ws(coupler, len(fields), coupler)
    fn, ctx = _torch_allreduce(coupler)
    with torch.cuda.device(coupler.device):
        check(capi.lib().mw_sponge_layer(C.byref(coupler.grid), _field_ptr_array(fields), len(fields), float(dt), float(time_scale),
                                         _ptr(ws), fn, ctx, _stream_ptr(coupler.device)))


class ColumnNudger:
    """modules::ColumnNudger, model/modules/column_nudging.h:9-108."""
    num_fields = 5

    def __init__(self):
        self.column = None

    @staticmethod
    def _state(coupler):
        dm = coupler.get_data_manager_readwrite()
        return [dm.get(n) for n in ("density_dry", "uvel", "vvel", "temp", "water_vapor")]

    def set_column(self, coupler):                                             # :15-36
        self.column = torch.zeros((5, coupler.get_nz(), coupler.get_nens()), dtype=torch.float64, device=coupler.device)
        ws = _column_ws(coupler, 5, self)
        fn, ctx = _torch_allreduce(coupler)
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_column_average(C.byref(coupler.grid), _field_ptr_array(self._state(coupler)), _ptr(self.column), _ptr(ws),
                                               fn, ctx, _stream_ptr(coupler.device)))

    def nudge_to_column(self, coupler, dt, defer_to=None):                     # :39-66
        """defer_to = the dycore module (round 6, no reference counterpart): the second pass -- state += dt (column - average) / 900 -- is not
        run; the increments are parked in the dycore handle and its next time_step adds them while it converts the coupler's fields (bit for
        bit the same result, one pass over five fields less per loop iteration).  Whoever reads a field through the DataManager in between
        triggers the pass after all (DataManager.before_access), so nobody ever SEES un-nudged values."""
        if self.column is None:
            endrun("ColumnNudger.nudge_to_column before set_column")
        ws = _column_ws(coupler, 5, self)
        fn, ctx = _torch_allreduce(coupler)
        state = self._state(coupler)
        with torch.cuda.device(coupler.device):
            if defer_to is not None:
                dm = coupler.get_data_manager_readwrite()
                if getattr(defer_to, "_flush_hook_dm", None) is not dm:
                    import weakref
                    ref = weakref.ref(defer_to)
                    dm.before_access.append(lambda: ref() is not None and ref().h and ref().flush_pending())
                    defer_to._flush_hook_dm = dm
                check(capi.lib().mw_nudge_to_column_deferred(defer_to.h, _field_ptr_array(state), _ptr(self.column), float(dt), _ptr(ws), fn, ctx))
                defer_to._parked = True
            else:
                check(capi.lib().mw_nudge_to_column(C.byref(coupler.grid), _field_ptr_array(state), _ptr(self.column), float(dt),
                                                    _ptr(ws), fn, ctx, _stream_ptr(coupler.device)))


# ---------------------------------------------------------------------------------------------------------------------
# File output and the simple_city custom modules (rank 3)
# ---------------------------------------------------------------------------------------------------------------------
def _barrier(coupler):
    import torch.distributed as dist
    if coupler.get_nranks() > 1 and dist.is_initialized():
        dist.barrier()


class _NcFile:
    """RAII wrapper over the mw_nc_* writer (CDF-5 by default, like the reference's NC_64BIT_DATA)."""

    def __init__(self, path, create, fmt=5, header_align=0, var_align=0):
        self.h = C.c_void_p(None)
        L = capi.lib()
        if create:
            check(L.mw_nc_create(C.byref(self.h), path.encode(), fmt, header_align, var_align))
        else:
            check(L.mw_nc_open(C.byref(self.h), path.encode()))

    def def_dim(self, name, n):
        d = C.c_int(-1)
        check(capi.lib().mw_nc_def_dim(self.h, name.encode(), int(n), C.byref(d)))
        return d.value

    def def_var(self, name, dims):
        v = C.c_int(-1)
        arr = (C.c_int * max(1, len(dims)))(*dims)
        check(capi.lib().mw_nc_def_var(self.h, name.encode(), len(dims), arr, C.byref(v)))
        return v.value

    def enddef(self):
        check(capi.lib().mw_nc_enddef(self.h))

    def varid(self, name):
        v = C.c_int(-1)
        check(capi.lib().mw_nc_inq_varid(self.h, name.encode(), C.byref(v)))
        return v.value

    def dimlen(self, name):
        n = C.c_longlong(-1)
        check(capi.lib().mw_nc_inq_dimlen(self.h, name.encode(), C.byref(n)))
        return n.value

    def def_var_typed(self, name, nc_type, dims):
        v = C.c_int(-1)
        arr = (C.c_int * max(1, len(dims)))(*dims)
        check(capi.lib().mw_nc_def_var_typed(self.h, name.encode(), nc_type, len(dims), arr, C.byref(v)))
        return v.value

    def put_typed(self, varid, start, count, data):
        """data: a contiguous numpy array of the variable's own type (int32 / float32 / float64)."""
        data = np.ascontiguousarray(data)
        st = (C.c_longlong * max(1, len(start)))(*start)
        ct = (C.c_longlong * max(1, len(count)))(*count)
        check(capi.lib().mw_nc_put_vara(self.h, varid, st, ct, data.ctypes.data_as(C.c_void_p)))

    def put(self, varid, start, count, data):
        data = np.ascontiguousarray(data, dtype=np.float64)
        st = (C.c_longlong * max(1, len(start)))(*start)
        ct = (C.c_longlong * max(1, len(count)))(*count)
        check(capi.lib().mw_nc_put_vara_double(self.h, varid, st, ct, data.ctypes.data_as(C.c_void_p)))

    def put_field(self, varid, record, coupler, tensor):
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_output_put_field(self.h, varid, record, C.byref(coupler.grid), _ptr(tensor), _stream_ptr(coupler.device)))

    def set_numrecs(self, n):
        check(capi.lib().mw_nc_set_numrecs(self.h, int(n)))

    def get(self, name, rec_start=0, rec_count=None):
        """Reads a variable back as a numpy array of its own type: a record variable's records [rec_start, rec_start + rec_count) (default:
        all) in full, record axis first, or the whole of a fixed-size variable (a scalar comes back with shape ())."""
        L = capi.lib()
        vid = self.varid(name)
        ty, nd, rec, shape = C.c_int(0), C.c_int(0), C.c_int(0), (C.c_longlong * 8)()
        check(L.mw_nc_inq_var(self.h, vid, C.byref(ty), C.byref(nd), shape, C.byref(rec)))
        dims = [int(shape[i]) for i in range(nd.value)]
        if rec.value:
            rec_count = dims[0] - int(rec_start) if rec_count is None else int(rec_count)
            dims[0] = rec_count
        out = np.empty(dims, dtype={4: np.int32, 5: np.float32, 6: np.float64}[ty.value])
        if out.size:
            check(L.mw_nc_get_var(self.h, vid, int(rec_start) if rec.value else 0, rec_count if rec.value else 0,
                                  out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if self.h and self.h.value:
            h, self.h = self.h, C.c_void_p(None)
            check(capi.lib().mw_nc_close(h))


def _coords(coupler):
    """x/y/z cell-centre coordinates of this rank's block (:2133-2147)."""
    g = coupler.grid
    dx, dy, dz = coupler.get_dx(), coupler.get_dy(), coupler.get_dz()
    return ((np.arange(g.nx) + g.i_beg + 0.5) * dx, (np.arange(g.ny) + g.j_beg + 0.5) * dy, (np.arange(g.nz) + 0.5) * dz)


def dycore_output(coupler, etime, fmt=5, barrier=None):
    """Dynamics_Euler_Stratified_WenoFV::output(coupler, etime), dynamics_euler_stratified_wenofv.h:2019-2191, shared-file
    branch (:2092-2188): one CDF-5 file `<out_prefix>.nc`, dims x,y,z (global sizes) and unlimited t, variables x,y,z,t and
    one (t,z,y,x) double variable per coupler field (ensemble member 0).  etime == 0 creates the file (main rank), later calls
    append a record.  `file_per_process` (:2038-2090): see _dycore_output_per_process."""
    if coupler.get_option("file_per_process", False):
        return _dycore_output_per_process(coupler, etime, fmt)
    barrier = barrier or (lambda: _barrier(coupler))
    path = str(coupler.get_option("out_prefix")) + ".nc"
    names = ["density_dry", "uvel", "vvel", "wvel", "temp"] + list(coupler.get_tracer_names())
    g = coupler.grid
    xs, ys, zs = _coords(coupler)
    main = coupler.is_mainproc()
    if etime == 0:
        if main:
            nc = _NcFile(path, True, fmt, 1048576, 1048576)                  # nc_header_align_size / nc_var_align_size, :2103-2104
            dx_, dy_, dz_ = nc.def_dim("x", coupler.get_nx_glob()), nc.def_dim("y", coupler.get_ny_glob()), nc.def_dim("z", g.nz)
            dt_ = nc.def_dim("t", 0)
            for n_, d_ in (("x", [dx_]), ("y", [dy_]), ("z", [dz_]), ("t", [dt_])):
                nc.def_var(n_, d_)
            for n_ in names:
                nc.def_var(n_, [dt_, dz_, dy_, dx_])
            nc.enddef()
            nc.put(nc.varid("z"), [0], [g.nz], zs)
            nc.put(nc.varid("t"), [0], [1], [0.0])
        barrier()
        if not main:
            nc = _NcFile(path, False)
        nc.put(nc.varid("x"), [g.i_beg], [g.nx], xs)
        nc.put(nc.varid("y"), [g.j_beg], [g.ny], ys)
        rec = 0
    else:
        nc = _NcFile(path, False)
        rec = nc.dimlen("t")
        if main:
            nc.put(nc.varid("t"), [rec], [1], [float(etime)])
    dm = coupler.get_data_manager_readonly()
    for n_ in names:
        nc.put_field(nc.varid(n_), rec, coupler, dm.get(n_))
    barrier()                                                                  # every rank's block is in the file ...
    if main:
        nc.set_numrecs(rec + 1)                                                # ... before the record becomes visible
    nc.close()
    barrier()


def _dycore_output_per_process(coupler, etime, fmt=5):
    """The `file_per_process` branch (:2038-2090): every rank writes `<out_prefix>_<rank, 8 digits>.nc` with its LOCAL x/y sizes
    and its own coordinate values; no communication.  (The reference's SimpleNetCDF produces a NetCDF-4 container here; this
    writer produces the classic CDF-5 layout with the same dimensions, variables and values.)"""
    path = "%s_%08d.nc" % (coupler.get_option("out_prefix"), coupler.get_myrank())
    names = ["density_dry", "uvel", "vvel", "wvel", "temp"] + list(coupler.get_tracer_names())
    g = coupler.grid
    xs, ys, zs = _coords(coupler)
    local = capi.Grid.from_buffer_copy(g)                                       # hyperslab offsets are local in a per-rank file
    local.i_beg, local.j_beg = 0, 0
    if etime == 0:
        nc = _NcFile(path, True, fmt)
        dx_, dy_, dz_, dt_ = nc.def_dim("x", g.nx), nc.def_dim("y", g.ny), nc.def_dim("z", g.nz), nc.def_dim("t", 0)
        for n_, d_ in (("x", [dx_]), ("y", [dy_]), ("z", [dz_]), ("t", [dt_])):
            nc.def_var(n_, d_)
        for n_ in names:
            nc.def_var(n_, [dt_, dz_, dy_, dx_])
        nc.enddef()
        nc.put(nc.varid("x"), [0], [g.nx], xs); nc.put(nc.varid("y"), [0], [g.ny], ys); nc.put(nc.varid("z"), [0], [g.nz], zs)
        rec = 0
    else:
        nc = _NcFile(path, False)
        rec = nc.dimlen("t")
    nc.put(nc.varid("t"), [rec], [1], [float(etime)])
    dm = coupler.get_data_manager_readonly()
    for n_ in names:
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_output_put_field(nc.h, nc.varid(n_), rec, C.byref(local), _ptr(dm.get(n_)), _stream_ptr(coupler.device)))
    nc.set_numrecs(rec + 1)
    nc.close()


Dynamics_Euler_Stratified_WenoFV.output = lambda self, coupler, etime, **kw: dycore_output(coupler, etime, **kw)

_SIX = ("density_dry", "uvel", "vvel", "wvel", "temp", "water_vapor")


class Horizontal_Sponge:
    """custom_modules::Horizontal_Sponge, experiments/simple_city/custom_modules/horizontal_sponge.h:7-194."""

    def __init__(self):
        self.column = None                                                     # (6, nz, nens): col_rho_d .. col_rho_v
        self.sponge_cells, self.time_scale = 10, 1.0

    def init(self, coupler, sponge_cells=10, time_scale=1.0):                  # :18-91
        dm = coupler.get_data_manager_readonly()
        self.column = torch.zeros((6, coupler.get_nz(), coupler.get_nens()), dtype=torch.float64, device=coupler.device)
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_horizontal_sponge_column(C.byref(coupler.grid), _field_ptr_array([dm.get(n) for n in _SIX]),
                                                         _ptr(self.column), _stream_ptr(coupler.device)))
        import torch.distributed as dist
        if coupler.get_nranks() > 1 and dist.is_initialized():                 # MPI_Bcast from the main rank, :73-78
            if dist.get_backend() == "gloo":
                h = self.column.cpu(); dist.broadcast(h, 0); self.column.copy_(h)
            else:
                dist.broadcast(self.column, 0)
        self.sponge_cells, self.time_scale = int(sponge_cells), float(time_scale)

    def _override(self, l, val):
        self.column[l].fill_(float(val))

    def override_rho_d(self, val): self._override(0, val)                      # noqa: E704   :94-99
    def override_uvel(self, val): self._override(1, val)                       # noqa: E704
    def override_vvel(self, val): self._override(2, val)                       # noqa: E704
    def override_wvel(self, val): self._override(3, val)                       # noqa: E704
    def override_temp(self, val): self._override(4, val)                       # noqa: E704
    def override_rho_v(self, val): self._override(5, val)                      # noqa: E704

    def apply(self, coupler, dt, x1=True, x2=True, y1=True, y2=True):          # :101-192
        if self.column is None:
            endrun("Horizontal_Sponge.apply before init")
        dm = coupler.get_data_manager_readwrite()
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_horizontal_sponge_apply(C.byref(coupler.grid), _field_ptr_array([dm.get(n) for n in _SIX]), _ptr(self.column),
                                                        self.sponge_cells, self.time_scale, float(dt), int(x1), int(x2), int(y1), int(y2),
                                                        _stream_ptr(coupler.device)))


class Time_Averager:
    """custom_modules::Time_Averager, experiments/simple_city/custom_modules/time_averager.h:7-143."""

    def __init__(self):
        self.etime = 0.0

    def init(self, coupler):                                                   # :10-35
        dm = coupler.get_data_manager_readwrite()
        shape = (coupler.get_nz(), coupler.get_ny(), coupler.get_nx(), coupler.get_nens())
        for n in _SIX:
            dm.register_and_allocate("time_avg_" + n, "", shape)
            dm.get("time_avg_" + n).zero_()
        self.etime = 0.0

    def accumulate(self, coupler, dt):                                         # :37-78
        dm = coupler.get_data_manager_readwrite()
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_time_average_accumulate(C.byref(coupler.grid), _field_ptr_array([dm.get(n) for n in _SIX]),
                                                        _field_ptr_array([dm.get("time_avg_" + n) for n in _SIX]), float(self.etime),
                                                        float(dt), _stream_ptr(coupler.device)))
        self.etime += dt

    def finalize(self, coupler, path="time_averaged_fields.nc", fmt=5, barrier=None):   # :80-141
        barrier = barrier or (lambda: _barrier(coupler))
        g = coupler.grid
        xs, ys, zs = _coords(coupler)
        if coupler.is_mainproc():
            nc = _NcFile(path, True, fmt)
            dx_, dy_, dz_ = nc.def_dim("x", coupler.get_nx_glob()), nc.def_dim("y", coupler.get_ny_glob()), nc.def_dim("z", g.nz)
            for n_, d_ in (("x", [dx_]), ("y", [dy_]), ("z", [dz_])):
                nc.def_var(n_, d_)
            for n_ in _SIX:
                nc.def_var(n_, [dz_, dy_, dx_])
            nc.enddef()
            nc.put(nc.varid("z"), [0], [g.nz], zs)
        barrier()
        if not coupler.is_mainproc():
            nc = _NcFile(path, False)
        nc.put(nc.varid("x"), [g.i_beg], [g.nx], xs)
        nc.put(nc.varid("y"), [g.j_beg], [g.ny], ys)
        dm = coupler.get_data_manager_readonly()
        for n_ in _SIX:
            nc.put_field(nc.varid(n_), -1, coupler, dm.get("time_avg_" + n_))
        nc.close()
        barrier()


class StatisticsGatherer:
    """custom_modules::StatisticsGatherer, experiments/supercell_kessler_surrogate/custom_modules/gather_micro_statistics.h:9-90:
    which share of the cells has active microphysics (input = the coupler cloned before micro.time_step, output = after)."""

    def __init__(self):
        self.numer, self.denom, self.num_out = 0.0, 0.0, 0
        self.last_mask = None

    def gather_micro_statistics(self, inp, out, dt, etime, keep_mask=False):    # :19-58
        names = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")
        a = [inp.get_data_manager_readonly().get(n, True) for n in names]
        b = [out.get_data_manager_readonly().get(n, True) for n in names]
        mask = torch.empty((inp.get_nz(), inp.get_ny(), inp.get_nx()), dtype=torch.uint8, device=inp.device) if keep_mask else None
        cnt = C.c_longlong(0)
        with torch.cuda.device(inp.device):
            check(capi.lib().mw_micro_active_count(C.byref(inp.grid), _field_ptr_array(a), _field_ptr_array(b),
                                                   C.c_void_p(mask.data_ptr()) if keep_mask else None, C.byref(cnt), _stream_ptr(inp.device)))
        self.last_mask = mask
        if etime > (self.num_out + 1) * 200:                                   # :54
            self.print(inp)
            self.num_out += 1
        self.numer += float(cnt.value)
        self.denom += float(inp.get_nz() * inp.get_ny() * inp.get_nx())
        return cnt.value

    def ratio(self, coupler):                                                  # MPI_Reduce(SUM) of numer and denom, :77-86
        import torch.distributed as dist
        v = torch.tensor([self.numer, self.denom], dtype=torch.float64)
        if coupler.get_nranks() > 1 and dist.is_initialized():
            v = v.to(coupler.device) if dist.get_backend() != "gloo" else v
            dist.all_reduce(v)
            v = v.cpu()
        return float(v[0] / v[1]) if float(v[1]) > 0 else float("nan")

    def print(self, coupler):
        r = self.ratio(coupler)
        if coupler.is_mainproc():
            print("*** Ratio Active ***:  %10.6e" % r, flush=True)

    def finalize(self, coupler):                                               # :89
        self.print(coupler)


def _sample_file_create(fname):
    """An empty sample file: DataGenerator's dimensions and variables (generate_micro_surrogate_data.h:17-33), all defined at once."""
    nc = _NcFile(fname, True, 5)
    ds, dvi, dst, dvo = nc.def_dim("nsamples", 0), nc.def_dim("num_vars_in", 5), nc.def_dim("sten_size", 2), nc.def_dim("num_vars_out", 4)
    for n in ("time_step_size", "dx", "dy", "dz", "xlen", "ylen", "zlen"):
        nc.def_var_typed(n, 6, [])
    nc.def_var_typed("only_two_dimensions", 4, [])
    nc.def_var_typed("inputs", 5, [ds, dvi, dst])
    nc.def_var_typed("outputs", 5, [ds, dvo])
    nc.enddef()
    nc.close()


def _sample_file_append(fname, coupler, dt, ins, outs, write_meta):
    """Appends host records ins (n, 5, 2), outs (n, 4) fp32 to a sample file (:116-153); write_meta: the grid's scalars first (:118-125,
    `if (!nc.varExists(..)) nc.write(..)`)."""
    n = int(ins.shape[0])
    nc = _NcFile(fname, False)
    ul = nc.dimlen("nsamples")                                                 # :116
    if write_meta:
        for name, val in (("time_step_size", dt), ("dx", coupler.get_dx()), ("dy", coupler.get_dy()), ("dz", coupler.get_dz()),
                          ("xlen", coupler.get_xlen()), ("ylen", coupler.get_ylen()), ("zlen", coupler.get_zlen())):
            nc.put_typed(nc.varid(name), [], [], np.array([val], dtype=np.float64))
        nc.put_typed(nc.varid("only_two_dimensions"), [], [], np.array([0 if coupler.get_ny_glob() == 1 else 1], dtype=np.int32))
    if n:
        nc.put_typed(nc.varid("inputs"), [ul, 0, 0], [n, 5, 2], np.ascontiguousarray(ins))
        nc.put_typed(nc.varid("outputs"), [ul, 0], [n, 4], np.ascontiguousarray(outs))
        nc.set_numrecs(ul + n)
    nc.close()


class DataGenerator:
    """custom_modules::DataGenerator, experiments/supercell_kessler_surrogate/custom_modules/generate_micro_surrogate_data.h:11-156:
    samples (5 inputs x 2-cell vertical stencil, 4 outputs; fp32) of the microphysics' effect, about half of them from active
    cells, appended to one file per rank.  The file is classic netCDF (CDF-5) instead of the reference's NetCDF-4 container, all
    variables are defined when it is created, and the random numbers come from splitmix64 (include/mw_cdna4.h)."""

    ratio_active = 0.4                       # :47-49 (from gather_statistics)
    desired_samples_per_time_step = 50.0     # :53
    desired_ratio_active = 0.5               # :55

    def init(self, coupler, directory="."):                                    # :17-33
        self.fname = os.path.join(directory, "supercell_kessler_data_task_%d.nc" % coupler.get_myrank())
        _sample_file_create(self.fname)
        self._meta_written = False
        if coupler.is_mainproc():
            with open(os.path.join(directory, "supercell_kessler_metadata.txt"), "w") as f:
                f.write("This dataset contains data for training a surrogate model to emulate Kessler microphysics.\n\n"
                        "vars_in : temperature, dry air density, water vapor density, cloud liquid density, precipitation density\n"
                        "vars_out: temperature, water vapor density, cloud liquid density, precipitation density\n")

    def generate_samples_stencil(self, inp, out, dt, etime, seed=None):        # :35-153
        import time as _time
        nx, ny, nz, nranks, myrank = inp.get_nx(), inp.get_ny(), inp.get_nz(), inp.get_nranks(), inp.get_myrank()
        ncell = nx * ny * nz
        want_act = self.desired_ratio_active * self.desired_samples_per_time_step / nranks          # :58-59
        want_inact = (1 - self.desired_ratio_active) * self.desired_samples_per_time_step / nranks
        thr_act = want_act / (self.ratio_active * ncell)                                             # :61-62
        thr_inact = want_inact / ((1 - self.ratio_active) * ncell)
        max_mag = (2 ** 64 - 1) // (nranks + ncell)                                                  # :84-85
        seed = (int(_time.time()) if seed is None else int(seed)) % max_mag
        key0 = ((seed + myrank) * ncell) % (2 ** 64)
        names = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")
        a = [inp.get_data_manager_readonly().get(n, True) for n in names]
        b = [out.get_data_manager_readonly().get(n, True) for n in names]
        rho_d = inp.get_data_manager_readonly().get("density_dry", True)
        dev = inp.device
        mask = torch.empty(ncell, dtype=torch.uint8, device=dev)
        L = capi.lib()
        with torch.cuda.device(dev):
            check(L.mw_micro_sample_mask(C.byref(inp.grid), _field_ptr_array(a), _field_ptr_array(b), key0, thr_act, thr_inact,
                                         C.c_void_p(mask.data_ptr()), _stream_ptr(dev)))
            cells = torch.nonzero(mask).flatten().contiguous()                 # ascending = the reference's (k,j,i) loop order
            n = int(cells.numel())
            ins = torch.empty((n, 5, 2), dtype=torch.float32, device=dev)
            outs = torch.empty((n, 4), dtype=torch.float32, device=dev)
            check(L.mw_micro_gather_samples(C.byref(inp.grid), _ptr(rho_d), _field_ptr_array(a), _field_ptr_array(b),
                                            C.c_void_p(cells.data_ptr()), n, C.c_void_p(ins.data_ptr()), C.c_void_p(outs.data_ptr()),
                                            _stream_ptr(dev)))
        self.last_cells = cells.cpu().numpy()                                 # k*ny*nx + j*nx + i of the samples (diagnostic)
        _sample_file_append(self.fname, inp, dt, ins.cpu().numpy(), outs.cpu().numpy(), not self._meta_written)
        self._meta_written = True
        return n


def install_exchange(dycore, coupler, transport="rccl", group=None):
    """Picks the halo-exchange transport for a multi-rank run TOGETHER on all ranks: the built-in RCCL transport unless any
    rank cannot set it up, in which case every rank switches to the torch.distributed point-to-point transport (ranks on
    different transports would deadlock).  Returns the transport in use: "none" (one rank), "rccl" or "torch"."""
    import torch.distributed as dist
    if coupler.get_nranks() <= 1:
        return "none"
    dev = coupler.device if dist.get_backend(group) != "gloo" else "cpu"

    def any_rank(failed):
        flag = torch.tensor([1 if failed else 0], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
        return int(flag.item()) == 1

    if transport == "rccl":
        failed, why = False, ""
        if not capi.lib().mw_rccl_library_path(None):                        # checked BEFORE the collective communicator set-up
            failed, why = True, "no librccl available to libmw_cdna4"
        if any_rank(failed):
            transport = "torch"
        else:
            try:
                use_rccl_exchange(dycore, coupler, group)
            except MWError as e:
                failed, why = True, str(e)
            if any_rank(failed):
                transport = "torch"
        if failed:
            import sys
            print("rank %d: built-in RCCL transport unavailable (%s)" % (coupler.get_myrank(), why), file=sys.stderr)
    if transport == "torch":
        use_torch_distributed_exchange(dycore, coupler, group)                # replaces (and frees) a half-installed RCCL transport
    return transport


def use_rccl_exchange(dycore, coupler, group=None):
    """Slab halo exchange over RCCL point-to-point inside the library (mw_rccl.cpp): rank 0 creates the ncclUniqueId,
    torch.distributed broadcasts it, every rank joins.  Replaces the MPI_Isend/Irecv of halo_exchange (:641-723)."""
    import torch.distributed as dist
    L = capi.lib()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    # 128 id bytes + 1 status byte.  Rank 0 ALWAYS reaches the broadcast -- with status 1 and a zero id when it could not create the
    # id -- and every rank raises only after it: a rank that left before the collective would leave the others waiting in it.
    ident = torch.zeros(129, dtype=torch.uint8, device=coupler.device)
    why = ""
    if rank == 0:
        buf = C.create_string_buffer(128)
        if L.mw_rccl_unique_id(buf) != 0:
            why = L.mw_last_error().decode(errors="replace")
            ident[128] = 1
        else:
            ident[:128].copy_(torch.tensor(list(buf.raw), dtype=torch.uint8))
    dist.broadcast(ident, 0, group=group)
    host = ident.cpu().tolist()
    if host[128]:
        raise MWError("rank 0 could not create the ncclUniqueId" + (": " + why if why else ""))
    with torch.cuda.device(coupler.device):
        check(L.mw_dycore_use_rccl(dycore.h, bytes(host[:128]), world, rank))


def use_rccl_self_exchange(dycore, coupler):
    """The self-loop test transport (mw_dycore_use_rccl_self): this one rank plays every rank of the coupler's rank grid over a 1-rank
    RCCL communicator -- the real send / receive groups on the side stream(s), on one GPU.  The column modules' sums go through the
    handle's communicator too (times the number of blocks)."""
    with torch.cuda.device(coupler.device):
        check(capi.lib().mw_dycore_use_rccl_self(dycore.h))
    use_rccl_allreduce(coupler, dycore)


def use_torch_distributed_exchange(dycore, coupler, group=None, host_staged=False):
    """Alternative transport for the same exchange: torch.distributed point-to-point ops (backend "nccl" = RCCL) issued
    from the library's exchange callback in the order of mw_exchange_plan.  Same wire pattern as the built-in transport.
    host_staged=True copies the strips through host buffers first -- the reference's non-GPU-aware-MPI mode
    (dynamics_euler_stratified_wenofv.h:687-722); works with the gloo backend."""
    import torch.distributed as dist
    L = capi.lib()
    peers, so, ro, act = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    check(L.mw_exchange_plan(C.byref(coupler.grid), peers, so, ro, act))
    dev = coupler.device

    def wrap(ptr, n):
        class _A:
            pass
        a = _A()
        a.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f8", data=(int(ptr), False), version=2)
        return torch.as_tensor(a, device=dev)

    def cb(ctx, sW, sE, sS, sN, rW, rE, rS, rN, nWE, nSN, stream):
        try:
            st = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
            with torch.cuda.device(dev), torch.cuda.stream(st):
                sb, rb, cnt = [sW, sE, sS, sN], [rW, rE, rS, rN], [nWE, nWE, nSN, nSN]
                if host_staged:
                    hs = {d: wrap(sb[d], cnt[d]).cpu() for d in range(4) if act[d] and cnt[d] and sb[d]}     # syncs the stream
                    hr = {d: torch.empty(cnt[d], dtype=torch.float64) for d in range(4) if act[d] and cnt[d] and rb[d]}
                    reqs = [dist.isend(hs[so[o]], peers[so[o]], group=group) for o in range(4) if so[o] in hs]
                    reqs += [dist.irecv(hr[ro[o]], peers[ro[o]], group=group) for o in range(4) if ro[o] in hr]
                    for r in reqs:
                        r.wait()
                    for d, t in hr.items():
                        wrap(rb[d], cnt[d]).copy_(t, non_blocking=False)
                    return 0
                ops = []
                for o in range(4):
                    d = so[o]
                    if act[d] and cnt[d] and sb[d]:
                        ops.append(dist.P2POp(dist.isend, wrap(sb[d], cnt[d]), peers[d], group))
                for o in range(4):
                    d = ro[o]
                    if act[d] and cnt[d] and rb[d]:
                        ops.append(dist.P2POp(dist.irecv, wrap(rb[d], cnt[d]), peers[d], group))
                if ops:
                    for r in dist.batch_isend_irecv(ops):
                        r.wait()
            return 0
        except Exception as e:                                   # pragma: no cover
            import sys
            print("exchange callback failed: %r" % (e,), file=sys.stderr)
            return 1

    dycore._xchg_cb = capi.EXCHANGE_FN(cb)                       # keep alive
    check(L.mw_dycore_set_exchange(dycore.h, dycore._xchg_cb, None))


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
