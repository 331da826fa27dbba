"""What every module of this host hands to the C ABI of include/mw_cdna4.h (no reference counterpart): device pointers of fp64 CUDA
tensors, the current stream, pointer arrays of field lists, and the two buffers that more than one module sizes from a C query -- the
workspace that grows on demand and the statistics-and-counts buffer that comes back in one copy."""
import ctypes as C

import numpy as np
import torch

from .capi import MWError


def _ptr(t):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise MWError("field tensors must be contiguous fp64 CUDA tensors")
    return C.c_void_p(t.data_ptr())


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _field_ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = _ptr(t).value
    return arr


def fit_workspace(ws, nbytes, device):
    """ws if it is an fp64 workspace of at least nbytes, else a new one that is."""
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
    return ws


def grown_workspace(holder, attr, nbytes, device):
    """The fp64 workspace kept as holder.<attr>: allocated at the first call, replaced by a larger one when a call needs more than it holds."""
    ws = fit_workspace(getattr(holder, attr, None), nbytes, device)
    setattr(holder, attr, ws)
    return ws


class StatsAndCounts:
    """n_f64 doubles followed by n_i64 int64 counts in ONE int64 device buffer: a kernel writes through stats_ptr and counts_ptr, host()
    fetches both with one device-to-host copy.  buf: the buffer of an earlier call of the same sizes, to use again."""

    def __init__(self, n_f64, n_i64, device, buf=None):
        self.n_f64 = int(n_f64)
        self.buf = torch.empty(self.n_f64 + int(n_i64), dtype=torch.int64, device=device) if buf is None else buf
        self.stats_ptr = C.c_void_p(self.buf.data_ptr())
        self.counts_ptr = C.c_void_p(self.buf.data_ptr() + 8 * self.n_f64)

    def host(self):
        """(the doubles, the counts) as flat numpy arrays of their own."""
        host = self.buf.cpu().numpy()
        return host[:self.n_f64].view(np.float64).copy(), host[self.n_f64:].copy()
