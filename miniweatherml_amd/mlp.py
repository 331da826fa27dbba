"""The Kessler surrogate network: its weight files and its forward passes, thin drivers of mw_mlp_* / mw_ponni_forward.

  load_h5_weights, load_surrogate_weights   experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h:97-135
  load_surrogate_model, SurrogateModel      the same files with the model's output form (no reference counterpart: DESIGN.md 13.9)
  mlp_forward, mlp_stencil_forward          model.forward_batch_parallel with the fused scaling, :176-202
  ponni_forward, _PonniLayer                ponni::create_inference_model / Inference::forward_batch_parallel, :109, :189

IN5 and OUT4 name the network's five input and four output fields in its order; every module that feeds or scores it takes them here."""
import collections
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import capi
from ._ffi import _ptr, _stream_ptr
from .capi import check
from .coupler import endrun

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
OUT4 = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")
BASE4 = (0, 2, 3, 4)                  # OUT4's fields among IN5: what an output replaces, and the base a tendency model's change is added to

# A model's OUTPUT FORM (MW_FORM_STATE / MW_FORM_TENDENCY, include/mw_cdna4.h): "state" -- the network's un-scaled output is the new state,
# the reference's form -- or "tendency" -- it is the change, added in fp64 to the cell's own temp, water_vapor, cloud_liquid, precip_liquid.
# The form travels with the files: a tendency model's output_scaling.txt starts with the comment line FORM_MARKER and its rows are the
# [min, max] of (after - before).
FORMS = ("state", "tendency")
FORM_MARKER = "# form: tendency"
SurrogateModel = collections.namedtuple("SurrogateModel", ("W1", "b1", "W2", "b2", "scl_in", "scl_out", "form"))


def form_code(form):
    """MW_FORM_* of a form given by name ("state" | "tendency") or by code (0 | 1); anything else is refused."""
    if isinstance(form, str) and form in FORMS:
        return FORMS.index(form)
    if isinstance(form, (int, np.integer)) and not isinstance(form, bool) and 0 <= int(form) < len(FORMS):
        return int(form)
    endrun("surrogate form: %r is neither of %r" % (form, FORMS))


def as_surrogate_model(model):
    """A SurrogateModel of what the consumers take: a 6-tuple (W1, b1, W2, b2, scl_in, scl_out) -- load_surrogate_weights' return, the
    state form -- or 7 fields with the form last."""
    m = tuple(model)
    if len(m) == 6:
        return SurrogateModel(*m, "state")
    if len(m) == 7:
        return SurrogateModel(*m[:6], FORMS[form_code(m[6])])
    endrun("surrogate model: a tuple of 6 (W1, b1, W2, b2, scl_in, scl_out) or 7 (+ form) expected, got %d" % len(m))


def read_form(out_scaling_txt):
    """The form an output scaling file declares: "tendency" if a comment line ahead of its rows is FORM_MARKER, else "state" (the
    reference's files and every file written before there were two forms carry no marker).  Another `# form:` value is refused."""
    with open(out_scaling_txt) as f:
        for line in f:
            t = line.strip()
            if t and not t.startswith("#"):
                break
            if t.startswith("# form:"):
                name = t[len("# form:"):].strip()
                if name not in FORMS:
                    endrun("%s: unknown output form %r (known: %s)" % (out_scaling_txt, name, ", ".join(FORMS)))
                return name
    return "state"


@contextlib.contextmanager
def strict_mode(strict):
    """mw_mlp_set_strict(strict) for the calls inside and 0 again behind them, also when one raises.  The caller checks a call's return
    code behind the block: the reset comes first."""
    check(capi.lib().mw_mlp_set_strict(int(bool(strict))))
    try:
        yield
    finally:
        check(capi.lib().mw_mlp_set_strict(0))


# (mlp_forward and mlp_stencil_forward below set the mode with a bare call and leave it set, as they always have -- every forward call sets
#  its own first.  That is kept on purpose: they do not use strict_mode.)
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
    """load_surrogate_model for callers that know only the state form: the six arrays, without the form.  Files of a tendency model are
    refused -- its marker is a comment, np.loadtxt would skip it, and the model would silently run as a state model."""
    m = load_surrogate_model(weights_txt, in_scaling_txt, out_scaling_txt, weights_h5)
    if m.form != "state":
        endrun("load_surrogate_weights: %s declares the %s form (%r); this function returns state-form models only -- read the files with "
               "mlp.load_surrogate_model, which returns the form with the arrays" % (out_scaling_txt, m.form, FORM_MARKER))
    return tuple(m[:6])


def load_surrogate_model(weights_txt=None, in_scaling_txt=None, out_scaling_txt=None, weights_h5=None):
    """The Keras weights + min/max scaling tables (microphysics_kessler_ponni.h:97-135).  weights_h5: the reference's
    `keras_weights_h5` file, read like ponni::load_h5_weights does (:103-107); weights_txt: a text export of the 104 values
    (tools/export_mlp_weights.sh).  Default: the reference's shipped weight file (miniweatherml_amd/data/).
    The model is inferred from the text files: 5 scaling rows + 104 weights = the single-cell model (W1 (5,10)), 9 rows + 144 weights = the
    two-cell stencil model (W1 (9,10); surrogate_train --stencil).  Any other pairing is refused; so is an .h5 file of a stencil model.
    Returns a SurrogateModel (W1, b1, W2, b2, scl_in, scl_out, form), the form read from the output scaling file (read_form)."""
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
    out_scaling_txt = out_scaling_txt or os.path.join(_DATA, "kessler_surrogate_output_scaling.txt")
    scl_out = np.loadtxt(out_scaling_txt, comments="#").reshape(4, 2)
    return SurrogateModel(W1, b1, W2, b2, np.ascontiguousarray(scl_in), np.ascontiguousarray(scl_out), read_form(out_scaling_txt))


def mlp_forward(temp, rho_d, rho_v, rho_c, rho_r, W1, b1, W2, b2, scl_in, scl_out, outs=None, strict=0, form="state"):
    """model.forward_batch_parallel with the fused scaling (microphysics_kessler_ponni.h:176-202).  strict = 1: the thread-per-cell
    form that accumulates in index order (bit-identical to the CPU restatement) instead of the MFMA kernels.  form="tendency": the
    un-scaled output is the change, added in fp64 to temp, rho_v, rho_c, rho_r of the cell (mw_mlp_forward_form)."""
    fc = form_code(form)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    if outs is None:
        outs = [torch.empty_like(temp) for _ in range(4)]
    check(capi.lib().mw_mlp_set_strict(int(bool(strict))))
    with torch.cuda.device(temp.device):
        check(capi.lib().mw_mlp_forward_form(fc, temp.numel(), _ptr(temp), _ptr(rho_d), _ptr(rho_v), _ptr(rho_c), _ptr(rho_r),
                                             W1.ctypes.data_as(fp), b1.ctypes.data_as(fp), W2.ctypes.data_as(fp), b2.ctypes.data_as(fp),
                                             scl_in.ctypes.data_as(dp), scl_out.ctypes.data_as(dp), *[_ptr(o) for o in outs],
                                             _stream_ptr(temp.device)))
    return outs


def mlp_stencil_forward(nz, temp, rho_d, rho_v, rho_c, rho_r, W1, b1, W2, b2, scl_in, scl_out, outs=None, strict=0, form="state"):
    """mlp_forward for the two-cell stencil model (W1 (9,10), scl_in (9,2)): the fields are whole coupler arrays (nz, ...) and features
    5..8 come from level min(nz - 1, k + 1) of the same column (stencil_features states the order).  The outputs never alias the inputs.
    form="tendency": the base of the change is level k's own value (mw_mlp_stencil_forward_form)."""
    fc = form_code(form)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    if W1.shape != (9, 10) or scl_in.shape != (9, 2):
        endrun("mlp_stencil_forward: W1 must be (9, 10) and scl_in (9, 2), got %r and %r" % (W1.shape, scl_in.shape))
    if temp.numel() % int(nz) != 0:
        endrun("mlp_stencil_forward: %d cells are not a whole number of columns of nz = %d" % (temp.numel(), nz))
    if outs is None:
        outs = [torch.empty_like(temp) for _ in range(4)]
    check(capi.lib().mw_mlp_set_strict(int(bool(strict))))
    with torch.cuda.device(temp.device):
        check(capi.lib().mw_mlp_stencil_forward_form(fc, int(nz), temp.numel() // int(nz), _ptr(temp), _ptr(rho_d), _ptr(rho_v), _ptr(rho_c),
                                                     _ptr(rho_r), W1.ctypes.data_as(fp), b1.ctypes.data_as(fp), W2.ctypes.data_as(fp),
                                                     b2.ctypes.data_as(fp), scl_in.ctypes.data_as(dp), scl_out.ctypes.data_as(dp),
                                                     *[_ptr(o) for o in outs], _stream_ptr(temp.device)))
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
    with strict_mode(strict), torch.cuda.device(x.device):
        rc = capi.lib().mw_ponni_forward(C.cast(arr, C.c_void_p), len(recs), flat.ctypes.data_as(C.POINTER(C.c_float)),
                                         int(sum(p.size for p in params)), x.shape[1], C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()),
                                         _stream_ptr(x.device))
    check(rc)
    return out


def load_training_domain(path, n_in):
    """A model's training_domain.txt (surrogate_train --init writes it): n_in rows `min max`, the range of each input
    over every sample the model and the models it continues were trained on.  Returns the (n_in, 2) fp64 array; a wrong row count, a
    NaN or a row with min > max is refused with the file's name."""
    import warnings
    try:
        with warnings.catch_warnings():                                        # (an empty file is refused below, by its shape)
            warnings.simplefilter("ignore")
            tab = np.atleast_2d(np.loadtxt(path, dtype=np.float64, comments="#"))
    except (OSError, ValueError) as e:
        endrun("training domain file %s: %s" % (path, e))
    if tab.shape != (int(n_in), 2):
        endrun("training domain file %s: %d rows of `min max` expected, it holds an array %r" % (path, int(n_in), tab.shape))
    if np.isnan(tab).any():
        endrun("training domain file %s: row %d holds a NaN" % (path, int(np.argwhere(np.isnan(tab))[0][0])))
    if (tab[:, 0] > tab[:, 1]).any():
        endrun("training domain file %s: row %d has min > max" % (path, int(np.argwhere(tab[:, 0] > tab[:, 1])[0][0])))
    return np.ascontiguousarray(tab)


def load_training_domains(entries, models):
    """Per entry of a `surrogate_models:` list None, or the table its `nn_training_domain` names (load_training_domain, with the row
    count of the entry's model in `models`): what domain_box takes as `tables`."""
    return [load_training_domain(e["nn_training_domain"], np.shape(m[4])[0]) if e.get("nn_training_domain") else None
            for e, m in zip(entries, models)]


def load_surrogate_bank(entries):
    """The models of a `surrogate_models:` list (dicts with keras_weights_txt | keras_weights_h5, nn_input_scaling, nn_output_scaling; `name`
    and other keys are ignored) as the list of SurrogateModel tuples that SurrogateBank takes; a model's form is its files'."""
    return [load_surrogate_model(weights_txt=e.get("keras_weights_txt"), in_scaling_txt=e.get("nn_input_scaling"),
                                   out_scaling_txt=e.get("nn_output_scaling"), weights_h5=e.get("keras_weights_h5")) for e in entries]
