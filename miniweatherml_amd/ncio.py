"""File output: the NetCDF writer of the library (mw_nc_*, csrc/mw_netcdf.cpp) as a file class, and what is written through it.

  dycore_output            Dynamics_Euler_Stratified_WenoFV::output, model/modules/dynamics_euler_stratified_wenofv.h:2019-2191
                           (shared file :2092-2188, file per process :2038-2090, coordinates :2133-2147)
  create_grid_file         the x/y/z(/t) file that output and Time_Averager::finalize
                           (experiments/simple_city/custom_modules/time_averager.h:80-141) both start from
  sample_file_create/_append   DataGenerator's file, experiments/supercell_kessler_surrogate/custom_modules/
                           generate_micro_surrogate_data.h:17-33 and :116-153

This module knows the coupler and the C ABI, not the modules that write through it."""
import ctypes as C

import numpy as np
import torch

from . import capi
from ._ffi import _ptr, _stream_ptr
from .capi import check


def _barrier(coupler):
    import torch.distributed as dist
    if coupler.get_nranks() > 1 and dist.is_initialized():
        dist.barrier()


class NcFile:
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

    def put_field(self, varid, record, coupler, tensor, grid=None):
        """This rank's block of a (.., z, y, x) variable from a coupler field (member 0); grid: whose offsets place it (default: the coupler's)."""
        with torch.cuda.device(coupler.device):
            check(capi.lib().mw_output_put_field(self.h, varid, record, C.byref(coupler.grid if grid is None else grid), _ptr(tensor),
                                                 _stream_ptr(coupler.device)))

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


def create_grid_file(path, coupler, names, record, fmt=5, align=0, shared=True, barrier=None):
    """A new file with the dimensions x, y, z (and the unlimited t with `record`), their coordinate variables and one double variable
    over (t,) z, y, x per name, the coordinates written; returns it open.  shared: ONE file of the global sizes -- the main rank creates
    it (align: its nc_header_align_size / nc_var_align_size) while the others wait at `barrier` and then open it, and every rank writes
    the x and y of its block; else a file of this rank's own sizes that it creates itself, no communication."""
    g = coupler.grid
    xs, ys, zs = _coords(coupler)
    main = coupler.is_mainproc()
    nx, ny, x0, y0 = (coupler.get_nx_glob(), coupler.get_ny_glob(), g.i_beg, g.j_beg) if shared else (g.nx, g.ny, 0, 0)
    if main or not shared:
        nc = NcFile(path, True, fmt, align, align)
        dims = [nc.def_dim("x", nx), nc.def_dim("y", ny), nc.def_dim("z", g.nz)] + ([nc.def_dim("t", 0)] if record else [])
        for n_, d_ in zip("xyzt", dims):
            nc.def_var(n_, [d_])
        for n_ in names:
            nc.def_var(n_, dims[::-1])
        nc.enddef()
        nc.put(nc.varid("z"), [0], [g.nz], zs)
    if shared:
        barrier()
        if not main:
            nc = NcFile(path, False)
    nc.put(nc.varid("x"), [x0], [g.nx], xs)
    nc.put(nc.varid("y"), [y0], [g.ny], ys)
    return nc


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
    main = coupler.is_mainproc()
    if etime == 0:
        nc = create_grid_file(path, coupler, names, True, fmt, 1048576, True, barrier)     # the alignments: :2103-2104
        rec = 0
    else:
        nc = NcFile(path, False)
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
    local = capi.Grid.from_buffer_copy(coupler.grid)                            # hyperslab offsets are local in a per-rank file
    local.i_beg, local.j_beg = 0, 0
    if etime == 0:
        nc = create_grid_file(path, coupler, names, True, fmt, shared=False)
        rec = 0
    else:
        nc = NcFile(path, False)
        rec = nc.dimlen("t")
    nc.put(nc.varid("t"), [rec], [1], [float(etime)])
    dm = coupler.get_data_manager_readonly()
    for n_ in names:
        nc.put_field(nc.varid(n_), rec, coupler, dm.get(n_), local)
    nc.set_numrecs(rec + 1)
    nc.close()


def sample_file_create(fname):
    """An empty sample file: DataGenerator's dimensions and variables (generate_micro_surrogate_data.h:17-33), all defined at once."""
    nc = NcFile(fname, True, 5)
    ds, dvi, dst, dvo = nc.def_dim("nsamples", 0), nc.def_dim("num_vars_in", 5), nc.def_dim("sten_size", 2), nc.def_dim("num_vars_out", 4)
    for n in ("time_step_size", "dx", "dy", "dz", "xlen", "ylen", "zlen"):
        nc.def_var_typed(n, 6, [])
    nc.def_var_typed("only_two_dimensions", 4, [])
    nc.def_var_typed("inputs", 5, [ds, dvi, dst])
    nc.def_var_typed("outputs", 5, [ds, dvo])
    nc.enddef()
    nc.close()


def sample_file_append(fname, coupler, dt, ins, outs, write_meta):
    """Appends host records ins (n, 5, 2), outs (n, 4) fp32 to a sample file (:116-153); write_meta: the grid's scalars first (:118-125,
    `if (!nc.varExists(..)) nc.write(..)`)."""
    n = int(ins.shape[0])
    nc = NcFile(fname, False)
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
