"""The Kessler surrogate network: its weight files and its forward passes, thin drivers of mw_mlp_* / mw_ponni_forward.

  load_h5_weights, load_surrogate_weights   experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h:97-135
  load_surrogate_model, SurrogateModel      the same files with the model's output form (no reference counterpart: DESIGN.md 13.9)
  mlp_forward, mlp_stencil_forward          model.forward_batch_parallel with the fused scaling, :176-202
  ponni_forward, _PonniLayer                ponni::create_inference_model / Inference::forward_batch_parallel, :109, :189
  SurrogateStack, load_surrogate_stack, write_surrogate_stack, stack_from_h5, MlpStack, mlp_stack_forward
                                            dense stacks of any width and depth (no reference counterpart: DESIGN.md 13.18)

IN5 and OUT4 name the network's five input and four output fields in its order; every module that feeds or scores it takes them here."""
import collections
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import capi
from ._ffi import StatsAndCounts, _field_ptr_array, _ptr, _stream_ptr, grown_workspace
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
               "weights (stencil model).  A dense stack of another shape declares it in a `# stack:` line and is read with "
               "mlp.load_surrogate_stack" % (rows if rows >= 0 else scl_in.size // 2, nw))
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


# ---- dense stacks n_in -> H1 -> ... -> HL -> 4 (mw_mlp_stack_*) ----
# A stack's weights file declares its shape in comment lines ahead of the numbers, which np.loadtxt skips: `# stack: 5 32 32 4` (n_in, the
# hidden widths, 4) and `# slopes: 0.1 0.1` (one leaky-ReLU slope per hidden layer); the numbers are the layers back to back in Keras
# order, W (in, out) then b per Dense.  The scaling files are the other models', the form marker included.
STACK_MARKER, SLOPES_MARKER = "# stack:", "# slopes:"
STACK_MAX_HIDDEN, STACK_MAX_WIDTH = 4, 64
SurrogateStack = collections.namedtuple("SurrogateStack", ("layers", "slopes", "scl_in", "scl_out", "form"))


def stack_header(weights_txt):
    """(widths, slopes) that the comment lines ahead of a weights file's numbers declare -- widths: [n_in, H1, .., HL, 4], slopes: a list
    of L floats or None without a `# slopes:` line -- or None for a file without a `# stack:` line (every file of the two fixed models)."""
    widths = slopes = None
    with open(weights_txt) as f:
        for line in f:
            t = line.strip()
            if t and not t.startswith("#"):
                break
            try:
                if t.startswith(STACK_MARKER):
                    widths = [int(w) for w in t[len(STACK_MARKER):].split()]
                elif t.startswith(SLOPES_MARKER):
                    slopes = [float(w) for w in t[len(SLOPES_MARKER):].split()]
            except ValueError:
                endrun("%s: the header line %r does not hold numbers" % (weights_txt, t))
    return None if widths is None else (widths, slopes)


def _stack_checked(stack, what):
    """The stack with float32 (W, b) layers, float32 slopes and float64 scaling tables, its shape checked against the limits of
    mw_mlp_stack_create (which checks them again: this is where the message names the file or the argument)."""
    layers, slopes, scl_in, scl_out, form = stack
    layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in layers]
    slopes = np.ascontiguousarray(slopes, dtype=np.float32).ravel()
    scl_in, scl_out = np.ascontiguousarray(scl_in, dtype=np.float64), np.ascontiguousarray(scl_out, dtype=np.float64)
    widths = [layers[0][0].shape[0]] + [b.size for _, b in layers] if layers and layers[0][0].ndim == 2 else []
    if not widths or len(layers) < 2 or len(layers) > STACK_MAX_HIDDEN + 1 or widths[0] not in (5, 9) or widths[-1] != 4 or \
            any(not 1 <= w <= STACK_MAX_WIDTH for w in widths[1:-1]):
        endrun("%s: a stack is n_in (5 or 9) -> 1 to %d hidden layers of 1 to %d units -> 4, got %r" % (what, STACK_MAX_HIDDEN, STACK_MAX_WIDTH, widths))
    for l, (W, b) in enumerate(layers):
        if W.shape != (widths[l], widths[l + 1]) or b.shape != (widths[l + 1],):
            endrun("%s: layer %d holds W %r and b %r, the widths %r need W (%d, %d)" % (what, l, W.shape, b.shape, widths, widths[l], widths[l + 1]))
    if slopes.size != len(layers) - 1 or not np.all(np.isfinite(slopes)) or np.any(slopes < 0):
        endrun("%s: one finite slope >= 0 per hidden layer expected (%d), got %r" % (what, len(layers) - 1, slopes.tolist()))
    if scl_in.shape != (widths[0], 2) or scl_out.shape != (4, 2):
        endrun("%s: scaling tables (%d, 2) and (4, 2) expected for n_in = %d, got %r and %r" % (what, widths[0], widths[0], scl_in.shape, scl_out.shape))
    return SurrogateStack(layers, slopes, scl_in, scl_out, FORMS[form_code(form)])


def stack_widths(stack):
    """[n_in, H1, .., HL, 4] of a SurrogateStack."""
    return [int(np.shape(stack.layers[0][0])[0])] + [int(np.size(b)) for _, b in stack.layers]


def load_surrogate_stack(weights_txt, in_scaling_txt, out_scaling_txt):
    """A SurrogateStack from a weights file with a `# stack:` / `# slopes:` header (write_surrogate_stack's) and the two scaling files;
    the form is the one the output scaling file declares (read_form).  A missing header, a number count that is not the header's, and
    scaling rows that are not n_in's are refused with the file's name."""
    head = stack_header(weights_txt)
    if head is None:
        endrun("%s: no `%s n_in H1 .. HL 4` line ahead of the numbers: not a stack's weights file (the two fixed models are read with "
               "mlp.load_surrogate_model)" % (weights_txt, STACK_MARKER))
    widths, slopes = head
    if slopes is None:
        endrun("%s: no `%s` line ahead of the numbers (one slope per hidden layer)" % (weights_txt, SLOPES_MARKER))
    if len(widths) < 3 or min(widths) < 1:
        endrun("%s: `%s` needs n_in, at least one hidden width and 4, all >= 1; it holds %r" % (weights_txt, STACK_MARKER, widths))
    w = np.atleast_1d(np.loadtxt(weights_txt, dtype=np.float64, comments="#")).astype(np.float32).ravel()
    need = sum((a + 1) * b for a, b in zip(widths[:-1], widths[1:]))
    if w.size != need:
        endrun("%s: the header %r declares %d weights, the file holds %d" % (weights_txt, widths, need, w.size))
    layers, off = [], 0
    for a, b in zip(widths[:-1], widths[1:]):
        layers.append((w[off:off + a * b].reshape(a, b).copy(), w[off + a * b:off + (a + 1) * b].copy()))
        off += (a + 1) * b
    scl_in = np.atleast_2d(np.loadtxt(in_scaling_txt, comments="#"))
    if scl_in.shape != (widths[0], 2):
        endrun("%s: %d rows of `min max` expected for the %d inputs that %s declares, it holds an array %r"
               % (in_scaling_txt, widths[0], widths[0], weights_txt, scl_in.shape))
    scl_out = np.atleast_2d(np.loadtxt(out_scaling_txt, comments="#"))
    if scl_out.shape != (4, 2):
        endrun("%s: 4 rows of `min max` expected, it holds an array %r" % (out_scaling_txt, scl_out.shape))
    return _stack_checked(SurrogateStack(layers, slopes, scl_in, scl_out, read_form(out_scaling_txt)), weights_txt)


def write_stack_weights(stack, path):
    """One weights file of a stack: the `# stack:` / `# slopes:` header, then the layers in Keras order, every number with the digits
    that restore its bits (the trainer's weights_<k>.txt are written with it)."""
    with open(path, "w") as f:
        f.write("%s %s\n" % (STACK_MARKER, " ".join(str(w) for w in stack_widths(stack))))
        f.write("%s %s\n" % (SLOPES_MARKER, " ".join(repr(float(s)) for s in stack.slopes)))     # (a float32 as a double: exact)
        for W, b in stack.layers:
            for v in np.concatenate([W.ravel(), b.ravel()]):
                f.write("%.9e\n" % v)


def write_surrogate_stack(stack, out_dir):
    """Writes weights.txt (with the header), input_scaling.txt and output_scaling.txt (with the form marker of a tendency model) into
    out_dir, every number with the digits that restore its bits; returns the three paths in load_surrogate_stack's order."""
    stack = _stack_checked(stack, "write_surrogate_stack")
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, n) for n in ("weights.txt", "input_scaling.txt", "output_scaling.txt")]
    write_stack_weights(stack, paths[0])
    for path, tab, marker in ((paths[1], stack.scl_in, False), (paths[2], stack.scl_out, stack.form == "tendency")):
        with open(path, "w") as f:
            if marker:
                f.write(FORM_MARKER + "\n")
            for lo, hi in tab:
                f.write("%.17e %.17e\n" % (lo, hi))
    return tuple(paths)


def stack_from_h5(path, dense_groups, slopes, in_scaling_txt=None, out_scaling_txt=None):
    """A SurrogateStack from the Dense layers of a Keras HDF5 weight file (load_h5_weights): dense_groups names them in order, e.g.
    ("dense_6", "dense_7") for the reference's shipped 5 -> 10 -> 4 file; slopes: one per hidden layer.  The scaling files default to the
    shipped tables; the form is the output scaling file's."""
    layers = []
    for gname in dense_groups:
        grp = "/%s/%s" % (gname, gname)
        layers.append((load_h5_weights(path, grp, "kernel:0"), load_h5_weights(path, grp, "bias:0")))
    out_scaling_txt = out_scaling_txt or os.path.join(_DATA, "kessler_surrogate_output_scaling.txt")
    scl_in = np.atleast_2d(np.loadtxt(in_scaling_txt or os.path.join(_DATA, "kessler_surrogate_input_scaling.txt"), comments="#"))
    scl_out = np.atleast_2d(np.loadtxt(out_scaling_txt, comments="#"))
    return _stack_checked(SurrogateStack(layers, slopes, scl_in, scl_out, read_form(out_scaling_txt)), str(path))


class MlpStack:
    """Owner of one mw_mlp_stack_t: the handle is created once (the operand images are built and uploaded to `device` then) and destroyed
    in close() / __del__."""

    def __init__(self, stack, device):
        self.stack = _stack_checked(stack, "MlpStack")
        self.device = torch.device(device)
        self.widths = stack_widths(self.stack)
        self._h = C.c_void_p()
        hidden = (C.c_int * (len(self.widths) - 2))(*self.widths[1:-1])
        params = np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in self.stack.layers]).astype(np.float32)
        fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
        with torch.cuda.device(self.device):
            check(capi.lib().mw_mlp_stack_create(C.byref(self._h), self.widths[0], len(hidden), hidden, self.stack.slopes.ctypes.data_as(fp),
                                                 params.ctypes.data_as(fp), params.size, self.stack.scl_in.ctypes.data_as(dp),
                                                 self.stack.scl_out.ctypes.data_as(dp), form_code(self.stack.form)))

    def forward(self, nz, temp, rho_d, rho_v, rho_c, rho_r, outs=None, strict=0):
        """mw_mlp_stack_forward on whole coupler arrays (nz, ...); n_in = 5 reads them as flat cells and may write in place."""
        if self._h is None or not self._h.value:
            endrun("MlpStack: the handle is closed")
        if temp.numel() % int(nz) != 0:
            endrun("mlp_stack_forward: %d cells are not a whole number of columns of nz = %d" % (temp.numel(), nz))
        if outs is None:
            outs = [torch.empty_like(temp) for _ in range(4)]
        with strict_mode(strict), torch.cuda.device(temp.device):
            rc = capi.lib().mw_mlp_stack_forward(self._h, int(nz), temp.numel() // int(nz), _ptr(temp), _ptr(rho_d), _ptr(rho_v), _ptr(rho_c),
                                                 _ptr(rho_r), *[_ptr(o) for o in outs], _stream_ptr(temp.device))
        check(rc)
        return outs

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            capi.lib().mw_mlp_stack_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


STACK_GROUP_MAX = 32


class MlpStackGroup:
    """Owner of one mw_stack_group_t: 1 to 32 stacks -- SurrogateStack tuples or MlpStack handles, n_in 5 and 9, any
    shapes and both forms mixed -- packed into device buffers of the group's own on `device`; members_apply rolls them out as ensemble
    members, evaluate scores them against the truth fields (with models, forms, n_ins and strict the group is a bank to
    surrogate_eval.SurrogateEvaluator).  The handle is destroyed in close() / __del__."""

    def __init__(self, stacks, device):
        self.device = torch.device(device)
        self._h = None
        stacks = list(stacks)
        if not 1 <= len(stacks) <= STACK_GROUP_MAX:
            endrun("MlpStackGroup: a group holds 1 to %d stacks, got %d" % (STACK_GROUP_MAX, len(stacks)))
        own = [None if isinstance(s, MlpStack) else MlpStack(s, self.device) for s in stacks]      # handles made for the packing alone
        handles = [s if o is None else o for s, o in zip(stacks, own)]
        self.stacks = [h.stack for h in handles]
        self.widths = [h.widths for h in handles]
        self.models = len(handles)                                        # what SurrogateEvaluator reads of a bank
        self.forms = [x.form for x in self.stacks]
        self.n_ins = [w[0] for w in self.widths]
        self.strict = 0                                                   # evaluate: 1 for the thread-per-cell kernel (mw_mlp_set_strict)
        self._buf = self._ws = self._cws = None
        h = C.c_void_p()
        try:
            if any(x._h is None or not x._h.value for x in handles):
                endrun("MlpStackGroup: a stack's handle is closed")
            with torch.cuda.device(self.device):
                check(capi.lib().mw_stack_group_create(C.byref(h), len(handles), (C.c_void_p * len(handles))(*[x._h.value for x in handles])))
        finally:
            for o in own:
                if o is not None:
                    o.close()
        self._h = h

    def members_apply(self, nz, members, fields5, strict=0):
        """mw_stack_group_members_apply: stack j replaces temp and the three water fields of ensemble member members[j] of the coupler's
        member-fastest arrays fields5 = (temp, density_dry, water_vapor, cloud_liquid, precip_liquid), each (nz, ..., nens), in place, with
        the bits MlpStack.forward writes for that member's own values (strict = 1: those of its thread-per-cell form)."""
        if self._h is None or not self._h.value:
            endrun("MlpStackGroup: the handle is closed")
        members = [int(m) for m in members]
        if len(members) != len(self.stacks):
            endrun("MlpStackGroup.members_apply: %d members for %d stacks" % (len(members), len(self.stacks)))
        f = fields5[0] if len(fields5) == 5 else None
        if f is None or f.dim() < 2 or any(t.shape != f.shape or t.device != f.device for t in fields5):
            endrun("MlpStackGroup.members_apply: five fields of one shape (nz, ..., nens) on one device expected")
        nens = int(f.shape[-1])
        n = f.numel() // nens
        if int(nz) < 1 or n % int(nz) != 0:
            endrun("MlpStackGroup.members_apply: %d cells per member are not a whole number of columns of nz = %d" % (n, nz))
        with strict_mode(strict), torch.cuda.device(f.device):
            rc = capi.lib().mw_stack_group_members_apply(self._h, (C.c_int * len(members))(*members), int(nz), n // int(nz), nens,
                                                         _field_ptr_array(list(fields5)), _stream_ptr(f.device))
        check(rc)

    def evaluate(self, nz, in5, truth4):
        """mw_stack_group_eval: in5 the five fields before the microphysics call (IN5), truth4 the four after it (OUT4); fp64 tensors of
        nz levels on the group's device.  Returns (stats, counts) as SurrogateBank.evaluate does: the raw (n + 1, 2, 4, 4) fp64 array
        [stack | persistence][inactive, active][field][sum d, sum |d|, sum d^2, max |d|], row j the j-th stack given, and the int64 cells
        per class -- one device-to-host copy for both.  The workspace is kept from call to call and regrown when the shape grows."""
        if self._h is None or not self._h.value:
            endrun("MlpStackGroup: the handle is closed")
        who = "MlpStackGroup.evaluate: "
        if len(in5) != 5 or len(truth4) != 4:
            endrun(who + "five input fields and four truth fields expected")
        every = list(in5) + list(truth4)
        n = in5[0].numel()
        if int(nz) < 1 or n % int(nz) != 0 or any(t.numel() != n for t in every):
            endrun(who + "the nine fields must have one size, a whole number of columns of nz = %d levels" % nz)
        if any(t.device != self.device for t in every):
            endrun(who + "the group lives on %s, the fields on %s" % (self.device, sorted({str(t.device) for t in every})))
        ncol = n // int(nz)
        nbytes = int(capi.lib().mw_stack_group_eval_workspace_bytes(self._h, int(nz), ncol))
        if nbytes < 1:
            endrun(who + "nz = %d and %d columns are out of range" % (nz, ncol))
        ws = grown_workspace(self, "_ws", nbytes, self.device)
        buf = StatsAndCounts((self.models + 1) * 32, 2, self.device, self._buf)
        self._buf = buf.buf                                               # (the int64 tensor itself: kept from call to call)
        with strict_mode(self.strict), torch.cuda.device(self.device):
            rc = capi.lib().mw_stack_group_eval(self._h, int(nz), ncol, _field_ptr_array(in5), _field_ptr_array(truth4), buf.stats_ptr,
                                                buf.counts_ptr, _ptr(ws), _stream_ptr(self.device))
        check(rc)
        stats, counts = buf.host()
        return stats.reshape(self.models + 1, 2, 4, 4), counts

    def _committee_layout(self, who, nz, every):
        """(ncol, nens) of the member-fastest fields `every` of a committee call, or endrun: one shape (nz, ..., nens), contiguous
        float64, on the group's device."""
        if self._h is None or not self._h.value:
            endrun("MlpStackGroup: the handle is closed")
        if any(t.shape != every[0].shape for t in every) or every[0].dim() < 2:
            endrun(who + "fields of one shape (nz, ..., nens) expected")
        if any(t.dtype != torch.float64 or not t.is_contiguous() for t in every):
            endrun(who + "contiguous float64 fields expected")
        nens = int(every[0].shape[-1])
        n = every[0].numel() // nens
        if int(nz) < 1 or n % int(nz) != 0:
            endrun(who + "%d cells per member are not a whole number of columns of nz = %d" % (n, nz))
        dev = every[0].device                                             # (a group made on "cuda" lives on the current device)
        if any(t.device != dev for t in every) or dev.type != self.device.type or self.device.index not in (None, dev.index):
            endrun(who + "the group lives on %s, the fields on %s" % (self.device, sorted({str(t.device) for t in every})))
        return n // int(nz), nens

    def committee_apply(self, nz, sel, member, in5, out4, range4=None):
        """mw_stack_group_committee_apply: the mean of the group's stacks sel (1 .. 16 distinct indices of one n_in, summed
        in that order) on ensemble member `member` of the member-fastest fields in5 = (temp, density_dry, water_vapor, cloud_liquid,
        precip_liquid), each (nz, ..., nens), written to out4 = (temp, water_vapor, cloud_liquid, precip_liquid) of the same shape -- each
        the matching input tensor (in place) or a tensor of its own -- and, with range4, the stacks' largest minus smallest value per cell
        and field: SurrogateBank.committee_apply for stacks.  Only elements of `member` are read and written (self.strict = 1: the
        thread-per-cell form).  A committee whose images do not fit the kernel's LDS together runs in chunks; their workspace is kept from
        call to call and regrown when the shape grows."""
        who = "MlpStackGroup.committee_apply: "
        sel = [int(s) for s in sel]
        if len(in5) != 5 or len(out4) != 4 or (range4 is not None and len(range4) != 4):
            endrun(who + "five input fields, four output fields and (optionally) four range fields expected")
        ncol, nens = self._committee_layout(who, nz, list(in5) + list(out4) + (list(range4) if range4 is not None else []))
        csel, nbytes = (C.c_int * max(1, len(sel)))(*sel), C.c_longlong(0)
        with strict_mode(self.strict), torch.cuda.device(self.device):
            rc = capi.lib().mw_stack_group_committee_workspace_bytes(self._h, len(sel), csel, int(nz), ncol, C.byref(nbytes))
            if rc == 0:
                ws = grown_workspace(self, "_cws", nbytes.value, self.device) if nbytes.value > 0 else None
                rc = capi.lib().mw_stack_group_committee_apply(self._h, len(sel), csel, int(member), int(nz), ncol, nens, _field_ptr_array(in5),
                                                               _field_ptr_array(out4), _field_ptr_array(range4) if range4 is not None else None,
                                                               _ptr(ws) if ws is not None else None, nbytes.value, _stream_ptr(self.device))
        check(rc)

    def committee_guard_flag(self, nz, sel, member, in5, thr4, guard, slot=0, domain_box=None):
        """mw_stack_group_committee_guard_flag: steps 1 and 2 of a guarded committee's step for ensemble member `member`
        in the committee's own last launch -- the mean of the stacks sel out of place into guard.mean4 (and guard.range4, when the
        CommitteeGuard keeps ranges), the member's bytes of guard.flags and row `slot` of guard.counts by mw_committee_guard_flags' rule
        with the thresholds thr4 (temp, water_vapor, cloud_liquid, precip_liquid; each >= 0, inf: never by size).  The state is only
        read.  SurrogateBank.committee_guard_flag's signature, so a rollout's loop calls either bank; stacks keep no training box and
        a domain_box is refused."""
        who = "MlpStackGroup.committee_guard_flag: "
        if domain_box is not None:
            endrun(who + "domain_box is not supported on a committee of stacks, which keep no training box")
        sel = [int(s) for s in sel]
        if len(in5) != 5 or len(thr4) != 4:
            endrun(who + "five input fields and four thresholds expected")
        ncol, nens = self._committee_layout(who, nz, list(in5))
        guard.check_layout(who, nz, in5[0], slot)
        csel, nbytes = (C.c_int * max(1, len(sel)))(*sel), C.c_longlong(0)
        thr = (C.c_double * 4)(*[float(t) for t in thr4])
        with strict_mode(self.strict), torch.cuda.device(self.device):
            rc = capi.lib().mw_stack_group_committee_workspace_bytes(self._h, len(sel), csel, int(nz), ncol, C.byref(nbytes))
            if rc == 0:
                ws = grown_workspace(self, "_cws", nbytes.value, self.device) if nbytes.value > 0 else None
                rc = capi.lib().mw_stack_group_committee_guard_flag(
                    self._h, len(sel), csel, int(member), int(nz), ncol, nens, _field_ptr_array(in5), _field_ptr_array(guard.mean4),
                    _field_ptr_array(guard.range4) if guard.range4 is not None else None, thr, C.c_void_p(guard.flags.data_ptr()),
                    C.c_void_p(guard.counts[slot].data_ptr()), _ptr(ws) if ws is not None else None, nbytes.value, _stream_ptr(self.device))
        check(rc)
        guard.flagged_members.add(int(member))

    def committee_guard_apply(self, nz, sel, member, in5, thr4, max_rainsplit, dz, dt, scratch, domain_box=None):
        """One step of a guarded committee of stacks on ensemble member `member`, in place (SurrogateBank.committee_guard_apply's
        contract and signature): committee_guard_flag into the scratch (a CommitteeGuard, with or without ranges), then
        CommitteeGuard.commit -- mw_kessler_columns_teacher on the flagged columns with out4 = mean4, mw_members_copy of mean4 into the
        four fields.  A scratch used for another member before has that member's flag bytes cleared first."""
        if scratch.flagged_members - {int(member)}:
            scratch.flags.zero_()
            scratch.flagged_members.clear()
        self.committee_guard_flag(nz, sel, member, in5, thr4, scratch, domain_box=domain_box)
        scratch.commit(nz, [member], in5, max_rainsplit, dz, dt)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            capi.lib().mw_stack_group_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mlp_stack_forward(stack_or_handle, nz, temp, rho_d, rho_v, rho_c, rho_r, outs=None, strict=0):
    """The forward pass of a dense stack on the coupler's fields: stack_or_handle is an MlpStack, or a SurrogateStack, for which a handle
    is created for this call and destroyed behind it (a loop keeps an MlpStack).  strict = 1: the thread-per-cell kernel in index order."""
    if isinstance(stack_or_handle, MlpStack):
        return stack_or_handle.forward(nz, temp, rho_d, rho_v, rho_c, rho_r, outs, strict)
    h = MlpStack(stack_or_handle, temp.device)
    try:
        outs = h.forward(nz, temp, rho_d, rho_v, rho_c, rho_r, outs, strict)
        torch.cuda.synchronize(temp.device)                                    # the handle's images are freed behind the call
    finally:
        h.close()
    return outs
