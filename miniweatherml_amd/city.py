"""The simple_city experiment's custom modules, thin drivers of mw_horizontal_sponge_* / mw_time_average_accumulate:

  Horizontal_Sponge   experiments/simple_city/custom_modules/horizontal_sponge.h:7-194
  Time_Averager       experiments/simple_city/custom_modules/time_averager.h:7-143"""
import ctypes as C

import torch

from . import capi
from ._ffi import _field_ptr_array, _ptr, _stream_ptr
from .capi import check
from .coupler import endrun
from .ncio import _barrier, create_grid_file

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
        nc = create_grid_file(path, coupler, _SIX, False, fmt, barrier=barrier)
        dm = coupler.get_data_manager_readonly()
        for n_ in _SIX:
            nc.put_field(nc.varid(n_), -1, coupler, dm.get("time_avg_" + n_))
        nc.close()
        barrier()
