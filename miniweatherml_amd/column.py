"""The column modules: horizontal means over all ranks and what is relaxed towards them, thin drivers of mw_sponge_layer / mw_column_* /
mw_nudge_to_column:

  sponge_layer    model/modules/sponge_layer.h:8-77
  ColumnNudger    model/modules/column_nudging.h:9-108"""
import ctypes as C

import torch

from . import capi
from ._ffi import _field_ptr_array, _ptr, _stream_ptr, grown_workspace
from .capi import check
from .coupler import endrun
from .exchange import _torch_allreduce


def _column_ws(coupler, nf, holder):
    return grown_workspace(holder, "_ws_col", capi.lib().mw_column_workspace_bytes(C.byref(coupler.grid), nf), coupler.device)


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
