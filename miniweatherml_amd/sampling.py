"""The surrogate experiment's statistics and training samples, thin drivers of mw_micro_*:

  StatisticsGatherer   experiments/supercell_kessler_surrogate/custom_modules/gather_micro_statistics.h:9-90
  DataGenerator        experiments/supercell_kessler_surrogate/custom_modules/generate_micro_surrogate_data.h:11-156

sample_thresholds and sample_buffers are what DataGenerator shares with the rollout's harvester: the threshold formulas (:61-62) and
nonzero plus the gather's buffers.  What differs stays with each: the C entry points, the meaning of an index (a cell of the grid there,
an element of the member layout here), the draw's key, and the harvester's clamp of its thresholds to 1."""
import ctypes as C
import os

import torch

from . import capi
from ._ffi import _field_ptr_array, _ptr, _stream_ptr
from .capi import check
from .mlp import OUT4
from .ncio import sample_file_append, sample_file_create


def sample_thresholds(want_active, want_inactive, prior_active, ncell):
    """generate_micro_surrogate_data.h:61-62: the probabilities with which an active and an inactive cell are drawn, so that ncell cells
    of which the share prior_active is active give about want_active + want_inactive samples."""
    return want_active / (prior_active * ncell), want_inactive / ((1 - prior_active) * ncell)


def sample_buffers(mask):
    """What a gather kernel takes for the cells a mask kernel marked, on the mask's device: their ascending indices (the reference's loop
    order) as int64, their number, and uninitialised fp32 inputs (n, 5, 2) and outputs (n, 4)."""
    cells = torch.nonzero(mask).flatten().contiguous()
    n = int(cells.numel())
    return cells, n, torch.empty((n, 5, 2), dtype=torch.float32, device=mask.device), torch.empty((n, 4), dtype=torch.float32, device=mask.device)


class StatisticsGatherer:
    """custom_modules::StatisticsGatherer, experiments/supercell_kessler_surrogate/custom_modules/gather_micro_statistics.h:9-90:
    which share of the cells has active microphysics (input = the coupler cloned before micro.time_step, output = after)."""

    def __init__(self):
        self.numer, self.denom, self.num_out = 0.0, 0.0, 0
        self.last_mask = None

    def gather_micro_statistics(self, inp, out, dt, etime, keep_mask=False):    # :19-58
        a = [inp.get_data_manager_readonly().get(n, True) for n in OUT4]
        b = [out.get_data_manager_readonly().get(n, True) for n in OUT4]
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
        sample_file_create(self.fname)
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
        thr_act, thr_inact = sample_thresholds(want_act, want_inact, self.ratio_active, ncell)      # :61-62
        max_mag = (2 ** 64 - 1) // (nranks + ncell)                                                  # :84-85
        seed = (int(_time.time()) if seed is None else int(seed)) % max_mag
        key0 = ((seed + myrank) * ncell) % (2 ** 64)
        a = [inp.get_data_manager_readonly().get(n, True) for n in OUT4]
        b = [out.get_data_manager_readonly().get(n, True) for n in OUT4]
        rho_d = inp.get_data_manager_readonly().get("density_dry", True)
        dev = inp.device
        mask = torch.empty(ncell, dtype=torch.uint8, device=dev)
        L = capi.lib()
        with torch.cuda.device(dev):
            check(L.mw_micro_sample_mask(C.byref(inp.grid), _field_ptr_array(a), _field_ptr_array(b), key0, thr_act, thr_inact,
                                         C.c_void_p(mask.data_ptr()), _stream_ptr(dev)))
            cells, n, ins, outs = sample_buffers(mask)                         # ascending = the reference's (k,j,i) loop order
            check(L.mw_micro_gather_samples(C.byref(inp.grid), _ptr(rho_d), _field_ptr_array(a), _field_ptr_array(b),
                                            C.c_void_p(cells.data_ptr()), n, C.c_void_p(ins.data_ptr()), C.c_void_p(outs.data_ptr()),
                                            _stream_ptr(dev)))
        self.last_cells = cells.cpu().numpy()                                 # k*ny*nx + j*nx + i of the samples (diagnostic)
        sample_file_append(self.fname, inp, dt, ins.cpu().numpy(), outs.cpu().numpy(), not self._meta_written)
        self._meta_written = True
        return n
