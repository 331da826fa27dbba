"""Native training of the Kessler surrogate (5 -> 10 -> 4, LeakyReLU(0.1)) from DataGenerator's sample files: the step of the reference's
surrogate workflow between generate_micro_data and inference_ponni, which the reference does in Keras
(experiments/supercell_kessler_surrogate/jupyter_notebooks/kessler_netcdf_to_numpy.ipynb, kessler_singlecell_train_example.ipynb).

    train_surrogate(sample_files, out_dir=None, epochs=10, batch_size=1024, ...) -> dict
    python -m miniweatherml_amd.surrogate_train FILE... --out DIR [--epochs N] [--models K] [--seed S] ...

The fit is the notebooks' recorded one, restated with integer-defined random choices (Keras' random streams cannot be reproduced):
pre-shuffle, per-variable min-max scaling over all samples, test split = the tail, validation split = the tail of the rest (Keras'
validation_split), per-epoch shuffle of the training set, Dense kernels uniform in [-0.05, 0.05), biases 0, loss mse, Nadam (TF 2.x Keras).
The hot path is csrc/mw_train.hip (one workgroup per model, the batches loop in the kernel); the validation and test predictions are
mw_ponni_forward's MFMA forward.  stencil=True (CLI --stencil) trains the two-cell stencil model 9 -> 10 -> 4 instead: the cell's five
inputs plus temperature, vapor, cloud and precipitation of the level above (STENCIL_IN_NAMES; slot 1 of the sample files), 144 parameters,
the same fit.  This file holds the host side: reading and checking the data, the permutations' definition (restated
here so that tests can replay the batch order), the Nadam scalars, the reports and the output files.  DESIGN.md section 13.
form="tendency" (CLI --tendency, with or without --stencil) trains the network on the CHANGE of the four output fields instead of their
new values: the labels are (after - before), scaled by the min and max of those differences, and the written model carries the form
(output_scaling.txt starts with `# form: tendency`); the network, the fit and every other file are the same.  DESIGN.md section 13.9.
file_weights / sample_weights (CLI --file-weights) is Keras' fit(sample_weight=...): the loss of a batch is sum_i w_i mean_o((y - t)^2) / B,
so that a small file -- a rollout's harvest beside the samples the model came from -- can count for more; group_metrics (CLI
--group-metrics) reports the validation and test errors of every file on its own.  DESIGN.md section 13.13.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

MAX_BATCH = 8192                     # MW_SURROGATE_MAX_BATCH (include/mw_cdna4.h)
MAX_MODELS = 256                     # MW_SURROGATE_MAX_MODELS
IN_NAMES = ("temperature", "dry air density", "water vapor density", "cloud liquid density", "precipitation density")
ABOVE_ROWS = (0, 1, 2, 3)            # rows of slot 1 that DataGenerator assigns (generate_micro_surrogate_data.h:139-142): row 4 never is
STENCIL_IN_NAMES = IN_NAMES + tuple(IN_NAMES[v] + " (level above)" for v in (0, 2, 3, 4))       # slot 1 has no dry density
OUT_NAMES = ("temperature", "water vapor density", "cloud liquid density", "precipitation density")
BASE_OF_OUT = (0, 2, 3, 4)           # the input that output j replaces: a tendency model's labels are outputs[:, j] - inputs[:, BASE_OF_OUT[j]]
FORMS = ("state", "tendency")        # mlp.FORMS / MW_FORM_STATE, MW_FORM_TENDENCY
FORM_MARKER = "# form: tendency"     # mlp.FORM_MARKER: the first line of a tendency model's output_scaling.txt
NADAM = dict(beta1=0.9, beta2=0.999, eps=1e-7, schedule_decay=0.004)    # tf.keras.optimizers.Nadam defaults
M64 = (1 << 64) - 1
TAG_PRESHUFFLE, TAG_WEIGHTS = M64, M64 - 1                               # stream tags; epoch e shuffles with tag e


class SurrogateTrainError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------------------------
# integer-defined random choices (the device side is csrc/mw_train.hip: make_feistel / feistel_index)
def splitmix64(z):
    z = (int(z) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def feistel_keys(a, tag, n):
    """Round keys and half width of the permutation of [0, n) for the stream (a, tag): base = sm64(sm64(a) ^ tag), key r = the high
    word of sm64(base + r), r = 0..3; h = the smallest h >= 1 with 4^h >= n."""
    base = splitmix64(splitmix64(int(a) & M64) ^ (int(tag) & M64))
    keys = [splitmix64((base + r) & M64) >> 32 for r in range(4)]
    h = 1
    while h < 32 and (1 << (2 * h)) < n:
        h += 1
    return keys, h


def feistel_permutation(n, a, tag):
    """perm[p] = the sample at position p: four Feistel rounds (L, R) <- (R, L ^ (mix32(R ^ key_r) & mask)) on x = (L << h) | R, applied
    again while the value is >= n (cycle-walking: a bijection of [0, n))."""
    keys, h = feistel_keys(a, tag, n)
    mask = np.uint32((1 << h) - 1)

    def rounds(x):
        L = (x >> np.uint64(h)).astype(np.uint32)
        R = (x & np.uint64(mask)).astype(np.uint32)
        for k in keys:
            L, R = R, L ^ (_mix32(R ^ np.uint32(k)) & mask)
        return (L.astype(np.uint64) << np.uint64(h)) | R.astype(np.uint64)

    out = rounds(np.arange(n, dtype=np.uint64))
    bad = np.flatnonzero(out >= np.uint64(n))
    while bad.size:
        out[bad] = rounds(out[bad])
        bad = bad[out[bad] >= np.uint64(n)]
    return out.astype(np.int64)


def preshuffle_permutation(n, seed):
    """kessler_netcdf_to_numpy.ipynb's shuffle of all samples: depends on the (split) seed alone."""
    return feistel_permutation(n, seed, TAG_PRESHUFFLE)


def epoch_permutation(n_train, seed, model, epoch):
    """The order in which model `model` visits the training set in epoch `epoch` (0-based): Keras' shuffle=True."""
    return feistel_permutation(n_train, (int(seed) + int(model)) & M64, int(epoch))


def n_params(stencil=False):
    """104 (single cell: W1 (5,10), b1 (10), W2 (10,4), b2 (4)) or 144 (stencil: W1 (9,10), ...)."""
    return 144 if stencil else 104


def split_weights(w):
    """W1, b1, W2, b2 of a flat parameter vector of either model (Keras order)."""
    w = np.asarray(w)
    n_in = {104: 5, 144: 9}[w.size]
    a = 10 * n_in
    return w[:a].reshape(n_in, 10), w[a:a + 10], w[a + 10:a + 50].reshape(10, 4), w[a + 50:a + 54]


def initial_weights(seed, models, stencil=False):
    """(models, 104 | 144) fp32: Dense kernels RandomUniform(-0.05, 0.05) -- u = (sm64(sm64(sm64(seed + m) ^ tag) + p) >> 40) / 2^24 for
    parameter index p, w = fp32(0.1 u - 0.05) -- and zero biases (Keras' defaults)."""
    npar = n_params(stencil)
    nw1 = npar - 54
    w = np.zeros((models, npar), dtype=np.float32)
    for m in range(models):
        base = splitmix64(splitmix64((int(seed) + m) & M64) ^ TAG_WEIGHTS)
        for p in list(range(0, nw1)) + list(range(nw1 + 10, nw1 + 50)):
            u = (splitmix64((base + p) & M64) >> 40) * (1.0 / 16777216.0)
            w[m, p] = np.float32(0.1 * u - 0.05)
    return w


def split_sizes(n, test_split=0.2, validation_split=0.2):
    """The notebook's int() arithmetic: n_fit = int((1 - test_split) n) samples are fitted, of which Keras keeps
    int(n_fit (1 - validation_split)) for training and validates on the rest.  Returns (n_train, n_val, n_test)."""
    n_fit = int((1.0 - test_split) * n)
    n_train = int(n_fit * (1.0 - validation_split))
    return n_train, n_fit - n_train, n - n_fit


def nadam_table(steps, learning_rate=1e-3, beta1=0.9, beta2=0.999, schedule_decay=0.004, first_step=0, dtype=np.float32):
    """Per-step scalars of Nadam (TF 2.x Keras) for steps first_step .. first_step + steps - 1, in fp64 then fp32: with t = step + 1,
    mu_t = beta1 (1 - 0.5 * 0.96^(decay t)), m_sched = prod mu_1..t;  [lr (1 - mu_t) / (1 - m_sched),  lr mu_t+1 / (1 - m_sched mu_t+1),
    1 - beta2^t].  The trainer takes them in fp32 (dtype)."""
    t_all = np.arange(1, first_step + steps + 1, dtype=np.float64)
    mu = beta1 * (1.0 - 0.5 * 0.96 ** (schedule_decay * t_all))
    mu_next = beta1 * (1.0 - 0.5 * 0.96 ** (schedule_decay * (t_all + 1.0)))
    sched = np.cumprod(mu)
    sl = slice(first_step, first_step + steps)
    tab = np.stack([learning_rate * (1.0 - mu[sl]) / (1.0 - sched[sl]),
                    learning_rate * mu_next[sl] / (1.0 - sched[sl] * mu_next[sl]),
                    1.0 - beta2 ** t_all[sl]], axis=1)
    return np.ascontiguousarray(tab, dtype=dtype)


def kernel_nadam_table(steps, learning_rate=1e-3, first_step=0):
    """The table the trainer's kernel takes.  The kernel receives beta2 as fp32 and runs v <- b v + (1 - b) g^2 with b = fp32(0.999) =
    0.999000013: 1 - b is exact in fp32 and 1.3e-5 (relative) below 1e-3.  The bias correction 1 - beta2^t must be the one of THAT
    recursion; built from 0.999 it leaves every sqrt(v_hat) 6.4e-6 too small, every step as much too long -- a one-sided error 50 times
    fp32's rounding, which adds up along the trajectory ("Gradient and trajectory accuracy").  beta1 needs no such
    care: Keras' Nadam corrects m with the momentum schedule, not with 1 - beta1^t."""
    return nadam_table(steps, learning_rate, NADAM["beta1"], float(np.float32(NADAM["beta2"])), NADAM["schedule_decay"], first_step)


# ---------------------------------------------------------------------------------------------------------------------------------
# data and arguments (host checks: they run before anything reaches the device)
def read_samples(sample_files, stencil=False):
    """Concatenates the files DataGenerator writes (CDF-5: inputs (nsamples, 5, 2), outputs (nsamples, 4) fp32) in the order given, through
    ncio.NcFile.  Returns inputs (n, 5) = slot 0 of the stencil (the single-cell model), outputs (n, 4), and the grid metadata.
    stencil=True: inputs (n, 9) = slot 0, then rows 0..3 of slot 1 (temperature, vapor, cloud and precipitation of the level above; its
    row 4 is never assigned and is not read).
    meta["file_index"] (n,) int32 is the position in `sample_files` of the file each sample came from, meta["file_counts"] the files' sizes."""
    from .ncio import NcFile
    if isinstance(sample_files, (str, os.PathLike)):
        sample_files = [sample_files]
    if not sample_files:
        raise SurrogateTrainError("no sample files given")
    ins, outs, meta = [], [], None
    for path in sample_files:
        nc = NcFile(os.fspath(path), False)
        try:
            i3, o2 = nc.get("inputs"), nc.get("outputs")
            m = {k: float(nc.get(k)) for k in ("time_step_size", "dx", "dy", "dz")}
        finally:
            nc.close()
        if i3.ndim != 3 or i3.shape[1:] != (5, 2) or o2.ndim != 2 or o2.shape[1] != 4 or o2.shape[0] != i3.shape[0]:
            raise SurrogateTrainError("%s: expected inputs (nsamples, 5, 2) and outputs (nsamples, 4)" % path)
        if meta is None:
            meta = m
        elif m["time_step_size"] != meta["time_step_size"]:
            raise SurrogateTrainError("%s: time_step_size %r differs from %r of %s; the Kessler outputs depend on dt, so files of "
                                      "different time steps cannot be trained together" % (path, m["time_step_size"],
                                                                                          meta["time_step_size"], sample_files[0]))
        ins.append(np.concatenate([i3[:, :, 0], i3[:, ABOVE_ROWS, 1]], axis=1) if stencil else np.ascontiguousarray(i3[:, :, 0]))
        outs.append(o2)
    inputs, outputs = np.concatenate(ins).astype(np.float32), np.concatenate(outs).astype(np.float32)
    meta["files"] = [os.fspath(p) for p in sample_files]
    meta["file_counts"] = [int(o.shape[0]) for o in outs]
    meta["file_index"] = np.repeat(np.arange(len(outs), dtype=np.int32), meta["file_counts"])
    return inputs, outputs, meta


def _check_form(form):
    if form not in FORMS:
        raise SurrogateTrainError("form must be one of %r, got %r" % (FORMS, form))
    return form


def tendencies(inputs, outputs):
    """(n, 4) fp64: what a tendency model is trained on, float64(outputs) - float64(inputs[:, BASE_OF_OUT]).  The records are fp32, so a
    change below the fp32 spacing of the value (temperature: 3e-5 K at 300 K) is 0 here."""
    return np.asarray(outputs, dtype=np.float64) - np.asarray(inputs, dtype=np.float64)[:, list(BASE_OF_OUT)]


def data_scaling(inputs, outputs, allow_constant=False, form="state"):
    """Refuses unusable data and returns the min-max tables scl_in (5 | 9, 2), scl_out (4, 2) (fp64 arrays holding the fp32 extremes).
    allow_constant (a warm start, whose tables are the continued model's): a constant variable is no refusal.
    form="tendency": scl_out is taken from tendencies(inputs, outputs), the differences in fp64; a constant difference is refused as a
    constant output is."""
    _check_form(form)
    if inputs.shape[0] == 0:
        raise SurrogateTrainError("the sample files hold zero samples")
    for arr, what in ((inputs, "inputs"), (outputs, "outputs")):
        bad = ~np.isfinite(arr)
        if bad.any():
            raise SurrogateTrainError("%d non-finite values in the %s (first at sample %d)" % (int(bad.sum()), what, int(np.argwhere(bad)[0][0])))
    tabs = []
    labels = tendencies(inputs, outputs) if form == "tendency" else outputs
    for arr, names, what in ((inputs, STENCIL_IN_NAMES if inputs.shape[1] == 9 else IN_NAMES, "input"),
                             (labels, OUT_NAMES, "output tendency" if form == "tendency" else "output")):
        lo, hi = arr.min(axis=0), arr.max(axis=0)
        for v in range(arr.shape[1]):
            if not hi[v] > lo[v] and not allow_constant:
                raise SurrogateTrainError("%s variable %d (%s) is constant (min = max = %r): its scaling (x - min) / (max - min) would "
                                          "divide by zero" % (what, v, names[v], float(lo[v])))
        tabs.append(np.ascontiguousarray(np.stack([lo, hi], axis=1).astype(np.float64)))
    return tabs[0], tabs[1]


def load_init(init, stencil=False):
    """The model a warm start continues: (weights (104 | 144,) fp32 in Keras order, scl_in, scl_out) from DIR/weights.txt,
    input_scaling.txt and output_scaling.txt (the files write_outputs leaves), read by mlp.load_surrogate_weights.  Host only.  The
    width must be the one that is trained.  The model's form is init_form's."""
    from .capi import MWError
    from .mlp import load_surrogate_model
    paths = [os.path.join(os.fspath(init), f) for f in ("weights.txt", "input_scaling.txt", "output_scaling.txt")]
    for path in paths:
        if not os.path.exists(path):
            raise SurrogateTrainError("init: no file %s" % path)
    try:
        W1, b1, W2, b2, scl_in, scl_out = load_surrogate_model(weights_txt=paths[0], in_scaling_txt=paths[1], out_scaling_txt=paths[2])[:6]
    except MWError as e:
        raise SurrogateTrainError("init: %s" % e)
    w = np.concatenate([np.ravel(W1), np.ravel(b1), np.ravel(W2), np.ravel(b2)]).astype(np.float32)
    if w.size != n_params(stencil):
        raise SurrogateTrainError("init: %s holds the %s model (%d parameters), but the %s model (%d) is trained%s"
                                  % (init, "stencil" if w.size == 144 else "single-cell", w.size, "stencil" if stencil else "single-cell",
                                     n_params(stencil), "" if stencil else " (--stencil trains the other)"))
    return w, np.ascontiguousarray(scl_in, dtype=np.float64), np.ascontiguousarray(scl_out, dtype=np.float64)


TRAINING_DOMAIN_FILE = "training_domain.txt"


def training_domain_union(data_rows, init_rows):
    """The rows of a continued model's training_domain.txt: per input the smaller of the two minima and the larger of
    the two maxima -- data_rows: data_scaling's input table of this run's samples; init_rows: the table of the model that is continued
    (init_domain).  (n_in, 2) fp64; pure numpy."""
    a, b = np.asarray(data_rows, dtype=np.float64), np.asarray(init_rows, dtype=np.float64)
    if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 2:
        raise SurrogateTrainError("training domain: this run's samples have the input table %r, the continued model's is %r" % (a.shape, b.shape))
    return np.ascontiguousarray(np.stack([np.minimum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])], axis=1))


def init_domain(init, n_in):
    """What the model in DIR was trained on, per input [min, max]: DIR/training_domain.txt if DIR's model was itself continued (the union
    over its ancestors), else DIR/input_scaling.txt, whose rows are the range of its own samples.  Host only."""
    from .capi import MWError
    from .mlp import load_training_domain
    path = os.path.join(os.fspath(init), TRAINING_DOMAIN_FILE)
    if not os.path.exists(path):
        path = os.path.join(os.fspath(init), "input_scaling.txt")
    if not os.path.exists(path):
        raise SurrogateTrainError("init: no file %s" % path)
    try:
        return load_training_domain(path, n_in)
    except MWError as e:
        raise SurrogateTrainError("init: %s" % e)


def write_training_domain(out_dir, rows):
    """training_domain.txt in out_dir: `min max` per input, in the scaling files' number format; returns its path."""
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, TRAINING_DOMAIN_FILE)
    with open(path, "w") as f:
        f.writelines("%s %s\n" % (_fmt(lo), _fmt(hi)) for lo, hi in np.asarray(rows))
    return path


def init_form(init):
    """The output form of the model in DIR (load_init's): what its output_scaling.txt declares, "state" without a marker.  Host only."""
    from .capi import MWError
    from .mlp import read_form
    path = os.path.join(os.fspath(init), "output_scaling.txt")
    if not os.path.exists(path):
        raise SurrogateTrainError("init: no file %s" % path)
    try:
        return read_form(path)
    except MWError as e:
        raise SurrogateTrainError("init: %s" % e)


def resolve_form(form, init):
    """The form a run trains: `form` ("state" | "tendency" | None = not asked for) without a warm start; with one, the form of DIR's model,
    and asking for the other form is refused either way round -- the weights were fitted to the other labels."""
    if form is not None:
        _check_form(form)
    if init is None:
        return form or "state"
    have = init_form(init)
    if form is not None and form != have:
        raise SurrogateTrainError("init: %s holds a %s-form model; it cannot be continued as a %s-form model%s"
                                  % (init, have, form, " (drop --tendency)" if form == "tendency" else " (it continues as tendency)"))
    return have


def check_arguments(n, epochs, batch_size, test_split, validation_split, models):
    if not (isinstance(batch_size, (int, np.integer)) and 1 <= batch_size <= MAX_BATCH):
        raise SurrogateTrainError("batch_size must be an integer in [1, %d], got %r" % (MAX_BATCH, batch_size))
    if not (isinstance(epochs, (int, np.integer)) and epochs >= 1):
        raise SurrogateTrainError("epochs must be an integer >= 1, got %r" % (epochs,))
    for name, v in (("test_split", test_split), ("validation_split", validation_split)):
        if not (0.0 < float(v) < 1.0):
            raise SurrogateTrainError("%s must be in (0, 1), got %r" % (name, v))
    if not (isinstance(models, (int, np.integer)) and 1 <= models <= MAX_MODELS):
        raise SurrogateTrainError("models must be an integer in [1, %d], got %r" % (MAX_MODELS, models))
    n_train, n_val, n_test = split_sizes(n, test_split, validation_split)
    for name, k in (("training", n_train), ("validation", n_val), ("test", n_test)):
        if k < 1:
            raise SurrogateTrainError("the %s set would be empty (%d samples, test_split %r, validation_split %r)" % (name, n, test_split,
                                                                                                                  validation_split))
    return n_train, n_val, n_test


def parse_file_weights(text):
    """The CLI's --file-weights: a comma list of floats, "1,1,25" -> (1.0, 1.0, 25.0)."""
    try:
        return tuple(float(t) for t in str(text).split(","))
    except ValueError:
        raise SurrogateTrainError("--file-weights: expected a comma list of numbers such as 1,1,25, got %r" % (text,))


def check_weights(n, file_index, n_files, file_weights=None, sample_weights=None):
    """The samples' weights (n,) fp32 in concatenated file order, or None when neither argument is given.  file_weights: one float per
    sample file; sample_weights: (n,).  Refused: both, a wrong count, a non-finite or a negative weight.  A weight of 0 is allowed."""
    if file_weights is None and sample_weights is None:
        return None
    if file_weights is not None and sample_weights is not None:
        raise SurrogateTrainError("file_weights and sample_weights are two ways to say the same thing: give one of them")
    what = "file_weights" if file_weights is not None else "sample_weights"
    try:
        w = np.asarray(file_weights if file_weights is not None else sample_weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise SurrogateTrainError("%s must be numbers" % what)
    want = n_files if file_weights is not None else n
    if w.ndim != 1 or w.size != want:
        raise SurrogateTrainError("%s: %d weights for %d %s" % (what, w.size, want, "sample files" if file_weights is not None else "samples"))
    if not np.isfinite(w).all():
        raise SurrogateTrainError("%s: non-finite weight (first at index %d)" % (what, int(np.flatnonzero(~np.isfinite(w))[0])))
    if (w < 0).any():
        raise SurrogateTrainError("%s: negative weight %r at index %d" % (what, float(w[w < 0][0]), int(np.flatnonzero(w < 0)[0])))
    w = w.astype(np.float32)
    return np.ascontiguousarray(w[file_index] if file_weights is not None else w)


def check_training_weights(w, n_train, split_seed):
    """Refuses weights that leave the training set without a positive one (every batch's loss would be zero).  The training set is the
    first n_train positions of the pre-shuffle; the permutation is only built when some weight is zero."""
    if w is None or (w > 0).all():
        return
    if not (w[preshuffle_permutation(w.size, split_seed)[:n_train]] > 0).any():
        raise SurrogateTrainError("no sample of the training set (%d of %d samples, split seed %d) has a positive weight: nothing would be "
                                  "trained" % (n_train, w.size, split_seed))


# ---------------------------------------------------------------------------------------------------------------------------------
# output files
def _fmt(v):
    return repr(float(v))                # shortest text that reads back to the same double (= the fp32 value)


def _write_weights(path, w, n_in):
    a = 10 * n_in
    with open(path, "w") as f:
        for title, lo, hi in (("dense_6 kernel (%d,10) row-major" % n_in, 0, a), ("dense_6 bias (10)", a, a + 10),
                              ("dense_7 kernel (10,4) row-major", a + 10, a + 50), ("dense_7 bias (4)", a + 50, a + 54)):
            f.write("# %s\n" % title)
            f.writelines(_fmt(x) + "\n" for x in w[lo:hi])


def write_outputs(out_dir, weights, scl_in, scl_out, history, all_weights=None, names=None, form="state"):
    """weights.txt (104 values, the layout of data/kessler_surrogate_weights.txt; 144 for the stencil model), input_scaling.txt /
    output_scaling.txt (`min max` rows, 5 | 9 and 4) and history.json; returns the three paths inference_ponni takes (keras_weights_txt,
    nn_input_scaling, nn_output_scaling).
    all_weights (models, 104 | 144): also weights_<k>.txt for every model k, in the same layout and beside the same two scaling files; the
    return value is then (paths, surrogate_models) with the `surrogate_models:` list of the evaluate_surrogates driver (names: the
    models' names, default model_<k>).
    form="tendency": output_scaling.txt starts with the line FORM_MARKER (its rows are the table of the differences); a state model's files
    are what they always were.  The readers are mlp.load_surrogate_model / read_form."""
    _check_form(form)
    os.makedirs(out_dir, exist_ok=True)
    w = np.asarray(weights, dtype=np.float32).ravel()
    n_in = np.asarray(scl_in).shape[0]
    if (n_in, w.size) not in ((5, 104), (9, 144)):
        raise SurrogateTrainError("write_outputs: %d input scaling rows with %d weights is neither the single-cell model (5, 104) nor the "
                                  "stencil model (9, 144)" % (n_in, w.size))
    paths = [os.path.join(out_dir, f) for f in ("weights.txt", "input_scaling.txt", "output_scaling.txt")]
    _write_weights(paths[0], w, n_in)
    for path, tab in ((paths[1], scl_in), (paths[2], scl_out)):
        with open(path, "w") as f:
            if path == paths[2] and form == "tendency":
                f.write(FORM_MARKER + "\n")
            f.writelines("%s %s\n" % (_fmt(lo), _fmt(hi)) for lo, hi in np.asarray(tab))
    with open(os.path.join(out_dir, "history.json"), "w") as f:
        json.dump(history, f, indent=1)
    if all_weights is None:
        return paths
    allw = np.asarray(all_weights, dtype=np.float32)
    if allw.ndim != 2 or allw.shape[1] != w.size:
        raise SurrogateTrainError("write_outputs: all_weights must be (models, %d), got %r" % (w.size, allw.shape))
    models = []
    for k in range(allw.shape[0]):
        path = os.path.join(out_dir, "weights_%d.txt" % k)
        _write_weights(path, allw[k], n_in)
        models.append({"name": str(names[k]) if names is not None else "model_%d" % k, "keras_weights_txt": path,
                       "nn_input_scaling": paths[1], "nn_output_scaling": paths[2]})
    return paths, models


# ---------------------------------------------------------------------------------------------------------------------------------
# the device side
def _layers(n_in):
    a = 10 * n_in
    return ((0, n_in, 10, 0.0, 0), (1, 10, 10, 0.0, a), (2, 10, 10, 0.1, 0), (0, 10, 4, 0.0, a + 10), (1, 4, 4, 0.0, a + 50))


_LAYERS = _layers(5)


class Trainer:
    """The device state of one training run: the three scaled sets, K models' parameters and moments, the Nadam table.  epoch() is one
    training launch plus the validation pass, with one host synchronisation (the copy of the weights and sums).  The model follows the
    data: raw_in (n, 5) trains the single-cell model (104 parameters), raw_in (n, 9) the stencil model (144).  form="tendency": the y sets
    are the scaled changes (mw_surrogate_prepare_form) and scl_out is the table of the changes; everything behind the prepare -- epochs,
    validation, test errors, predict_test -- works in scaled label space and is the same for both forms.
    sample_weights (n,): the samples' weights in the order of raw_in; they go through the same pre-shuffle and split
    (mw_surrogate_prepare_column), epoch() then runs mw_surrogate_train_epoch_w and validate() mw_surrogate_errors_weighted with the
    validation samples' weights, as Keras weights its validation split.  groups (n,): an integer label per sample (the index of its file),
    split the same way, for group_sums.  Without the two the trainer calls what it always called."""

    def __init__(self, raw_in, raw_out, scl_in, scl_out, n_split, seed=0, split_seed=None, models=1, batch_size=1024, epochs=10,
                 learning_rate=1e-3, initial=None, form="state", sample_weights=None, groups=None):
        import torch
        from . import capi
        self.torch, self.L = torch, capi.lib()
        self.device = raw_in.device
        self.form = _check_form(form)
        self.n_in = int(raw_in.shape[1])
        if self.n_in not in (5, 9) or np.asarray(scl_in).shape != (self.n_in, 2):
            raise SurrogateTrainError("Trainer: inputs (n, %d) with a scaling table %r; expected (n, 5) or (n, 9) and as many scaling rows"
                                      % (self.n_in, np.asarray(scl_in).shape))
        self.npar = NP = 54 + 10 * self.n_in
        self.n_train, self.n_val, self.n_test = n_split
        self.K, self.B, self.seed = int(models), int(batch_size), int(seed)
        self.split_seed = self.seed if split_seed is None else int(split_seed)
        self.steps = (self.n_train + self.B - 1) // self.B
        dev, f32 = self.device, torch.float32
        self.sets = {k: (torch.empty((self.n_in, n), dtype=f32, device=dev), torch.empty((4, n), dtype=f32, device=dev))
                     for k, n in (("train", self.n_train), ("val", self.n_val), ("test", self.n_test))}
        dp = C.POINTER(C.c_double)
        self.scl_in, self.scl_out = np.ascontiguousarray(scl_in, np.float64), np.ascontiguousarray(scl_out, np.float64)
        (tx, ty), (vx, vy), (sx, sy) = self.sets["train"], self.sets["val"], self.sets["test"]
        with torch.cuda.device(dev):
            capi.check(self.L.mw_surrogate_prepare_form(FORMS.index(self.form), self.n_in, raw_in.shape[0], self._p(raw_in), self._p(raw_out),
                                                        self.scl_in.ctypes.data_as(dp), self.scl_out.ctypes.data_as(dp), self.split_seed & M64,
                                                        self.n_train, self.n_val, *[self._p(t) for t in (tx, ty, vx, vy, sx, sy)], self._stream()))
        self.wsets = self._column(sample_weights, raw_in.shape[0])
        self.gsets = self._column(groups, raw_in.shape[0])
        self.n_groups = 0 if self.gsets is None else int(max(float(t.max()) for t in self.gsets.values())) + 1
        # ONE device buffer for what the host reads each epoch: parameters (K, 104) fp32 | training sums (K, 2) fp64 | validation sums (K, 24)
        self.buf = torch.zeros(self.K * (NP * 4 + 2 * 8 + 24 * 8), dtype=torch.uint8, device=dev)
        self.params = self.buf[:self.K * NP * 4].view(f32).view(self.K, NP)
        self.tstats = self.buf[self.K * NP * 4:self.K * (NP * 4 + 16)].view(torch.float64).view(self.K, 2)
        self.vstats = self.buf[self.K * (NP * 4 + 16):].view(torch.float64).view(self.K, 24)
        if initial is None:
            w0 = initial_weights(self.seed, self.K, stencil=self.n_in == 9)
        else:                                                              # a warm start: (K, npar), the moments and the step counter at zero
            w0 = np.ascontiguousarray(initial, dtype=np.float32)
            if w0.shape != (self.K, NP):
                raise SurrogateTrainError("Trainer: initial weights %r; expected (%d, %d)" % (w0.shape, self.K, NP))
        self.params.copy_(torch.from_numpy(w0))
        self.m1 = torch.zeros((self.K, NP), dtype=f32, device=dev)
        self.m2 = torch.zeros((self.K, NP), dtype=f32, device=dev)
        self.lr = float(learning_rate)
        self.table = torch.from_numpy(kernel_nadam_table(self.steps * int(epochs), self.lr)).to(dev)
        # validation predictions: groups of models whose (4, n_val) outputs fit in 1 GiB
        self.group = max(1, min(self.K, (1 << 30) // (16 * self.n_val)))
        self.pred = torch.empty(self.group * 4 * max(self.n_val, self.n_test), dtype=f32, device=dev)
        self.ws = torch.empty(int(self.L.mw_surrogate_errors_workspace_bytes(self.group)), dtype=torch.uint8, device=dev)
        self.test_out = torch.empty(24, dtype=torch.float64, device=dev)
        self.epoch_no = 0

    def _p(self, t):
        return C.c_void_p(t.data_ptr())

    def _column(self, col, n):
        """One value per sample, (n,) host or device, through the pre-shuffle and split: {"train": (n_train,), "val": ..., "test": ...} fp32."""
        if col is None:
            return None
        from . import capi
        torch = self.torch
        c = torch.as_tensor(col).to(device=self.device, dtype=torch.float32).contiguous()
        if c.shape != (n,):
            raise SurrogateTrainError("Trainer: a per-sample column of shape %r for %d samples" % (tuple(c.shape), n))
        out = {k: torch.empty(m, dtype=torch.float32, device=self.device) for k, m in (("train", self.n_train), ("val", self.n_val), ("test", self.n_test))}
        with torch.cuda.device(self.device):
            capi.check(self.L.mw_surrogate_prepare_column(n, self._p(c), self.split_seed & M64, self.n_train, self.n_val, self._p(out["train"]),
                                                          self._p(out["val"]), self._p(out["test"]), self._stream()))
        return out

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _predict(self, w104, x, out):
        from .capi import check
        from .mlp import _PonniLayer
        lay = (_PonniLayer * 5)(*[_PonniLayer(*r) for r in _layers(self.n_in)])
        w = np.ascontiguousarray(w104, dtype=np.float32)
        check(self.L.mw_ponni_forward(C.cast(lay, C.c_void_p), 5, w.ctypes.data_as(C.POINTER(C.c_float)), self.npar, x.shape[1], self._p(x),
                                      self._p(out), self._stream()))

    def _errors(self, n, nsets, pred, y, out_ptr, w=None):
        from .capi import check
        if w is None:
            check(self.L.mw_surrogate_errors(n, nsets, self._p(pred), self._p(y), self._p(self.ws), out_ptr, self._stream()))
        else:
            check(self.L.mw_surrogate_errors_weighted(n, nsets, self._p(pred), self._p(y), self._p(w), self._p(self.ws), out_ptr, self._stream()))

    def validate(self, weights):
        """Launches the validation pass of every model (weights: HOST (K, 104)); its sums land in vstats (read at the next copy)."""
        vx, vy = self.sets["val"]
        from .capi import check
        with self.torch.cuda.device(self.device):
            check(self.L.mw_mlp_set_strict(0))
            for g0 in range(0, self.K, self.group):
                ng = min(self.group, self.K - g0)
                pred = self.pred[:ng * 4 * self.n_val].view(ng, 4, self.n_val)
                for j in range(ng):
                    self._predict(weights[g0 + j], vx, pred[j])
                self._errors(self.n_val, ng, pred, vy, C.c_void_p(self.vstats.data_ptr() + g0 * 24 * 8),
                             None if self.wsets is None else self.wsets["val"])

    def epoch(self):
        """One training launch, ONE host synchronisation (a single copy of weights and sums), the validation launches.  Returns the host
        copy: weights (K, 104), this epoch's training sums (K, 2) and the PREVIOUS epoch's validation sums (K, 24)."""
        from .capi import check
        tx, ty = self.sets["train"]
        tail = (self.n_train, self.B, self.epoch_no, self.seed & M64, self._p(self.params), self._p(self.m1), self._p(self.m2),
                C.c_void_p(self.table.data_ptr() + self.epoch_no * self.steps * 12), NADAM["beta1"], NADAM["beta2"], NADAM["eps"],
                self._p(self.tstats), self._stream())
        with self.torch.cuda.device(self.device):
            if self.wsets is None:
                check(self.L.mw_surrogate_train_epoch_v2(self.n_in, self.K, self._p(tx), self._p(ty), *tail))
            else:
                check(self.L.mw_surrogate_train_epoch_w(self.n_in, self.K, self._p(tx), self._p(ty), self._p(self.wsets["train"]), *tail))
        host = self._host()
        self.validate(host[0])
        self.epoch_no += 1
        return host

    def _host(self):
        b = self.buf.cpu().numpy()
        K, nb = self.K, self.npar * 4
        return (b[:K * nb].view(np.float32).reshape(K, self.npar).copy(), b[K * nb:K * (nb + 16)].view(np.float64).reshape(K, 2).copy(),
                b[K * (nb + 16):].view(np.float64).reshape(K, 24).copy())

    def finish(self):
        """The last epoch's validation sums (one more copy)."""
        return self._host()

    def predict_test(self, w104):
        """The network's output for the test set, (4, n_test) fp32 on the device, in SCALED LABEL space: un-scaled with scl_out it is the
        new state of a state model, the change of a tendency model."""
        sx, _ = self.sets["test"]
        pred = self.torch.empty((4, self.n_test), dtype=self.torch.float32, device=self.device)
        with self.torch.cuda.device(self.device):
            self._predict(w104, sx, pred)
        return pred

    def test_errors(self, w104):
        sx, sy = self.sets["test"]
        pred = self.pred[:4 * self.n_test].view(4, self.n_test)
        with self.torch.cuda.device(self.device):
            self._predict(w104, sx, pred)
            self._errors(self.n_test, 1, pred, sy, self._p(self.test_out))
        return self.test_out.cpu().numpy().reshape(4, 6)

    def group_counts(self):
        """(n_groups, 3) int: every group's samples in the training, validation and test set, from the prepared label tensors."""
        return np.stack([self.torch.bincount(self.gsets[k].long(), minlength=self.n_groups).cpu().numpy() for k in ("train", "val", "test")], axis=1)

    def group_sums(self, w104, which):
        """The UNWEIGHTED error sums (4, 6) of every group's samples in the set `which` ("val" | "test") at the weights w104: one forward
        of the set, then one mw_surrogate_errors_weighted call per group with the group's indicator as weights.  None for an empty group."""
        x, y = self.sets[which]
        n = x.shape[1]
        pred = self.pred[:4 * n].view(4, n)
        out = []
        with self.torch.cuda.device(self.device):
            self._predict(w104, x, pred)
            for g in range(self.n_groups):
                ind = (self.gsets[which] == g).to(self.torch.float32)
                if not bool(ind.any()):
                    out.append(None)
                    continue
                self._errors(n, 1, pred, y, self._p(self.test_out), ind)
                out.append(self.test_out.cpu().numpy().reshape(4, 6).copy())
        return out


def _group_records(tr, w104, files, file_weights, unweighted):
    """train_surrogate's `group_metrics`: one record per file (see there)."""
    counts, vsum, tsum = tr.group_counts(), tr.group_sums(w104, "val"), tr.group_sums(w104, "test")
    out = []
    for g, path in enumerate(files):
        rec = {"file": path, "weight": 1.0 if unweighted else None if file_weights is None else float(file_weights[g]),
               "n_train": int(counts[g, 0]), "n_val": int(counts[g, 1]), "n_test": int(counts[g, 2])}
        v, t = vsum[g], tsum[g]
        rec["val_loss"] = None if v is None else float(v[:, 0].sum() / (4 * rec["n_val"]))
        rec["val_mean_absolute_error"] = None if v is None else float(v[:, 1].sum() / (4 * rec["n_val"]))
        rec["test_loss"] = None if t is None else float(t[:, 0].sum() / (4 * rec["n_test"]))
        m = None if t is None else _metrics(t)
        for k in ("max_relative_error", "mean_relative_error", "mean_relative_bias"):
            rec[k] = None if m is None else m[k]
        out.append(rec)
    return out


def group_line(g):
    """The CLI's line for one record of `group_metrics`."""
    num = lambda v: "none" if v is None else "%.4e" % v                  # noqa: E731
    return ("file %s (weight %s): train %d / val %d / test %d - val_loss: %s - val_mean_absolute_error: %s - test_loss: %s - "
            "mean relative errors: %s" % (g["file"], "per sample" if g["weight"] is None else "%g" % g["weight"], g["n_train"], g["n_val"],
                                          g["n_test"], num(g["val_loss"]), num(g["val_mean_absolute_error"]), num(g["test_loss"]),
                                          g["mean_relative_error"]))


def _metrics(s):
    """The notebook's test cell from the error sums of one set (4 outputs x [sum d^2, sum |d|, sum d, sum |o|, max |d|, max |o|])."""
    s = np.asarray(s, dtype=np.float64).reshape(4, 6)
    return {"max_relative_error": (s[:, 4] / s[:, 5]).tolist(), "mean_relative_error": (s[:, 1] / s[:, 3]).tolist(),
            "mean_relative_bias": (s[:, 2] / s[:, 3]).tolist()}


def train_surrogate(sample_files, out_dir=None, epochs=10, batch_size=1024, test_split=0.2, validation_split=0.2, learning_rate=1e-3,
                    seed=0, models=1, device="cuda:0", split_seed=None, verbose=False, stencil=False, keep_all=False, init=None, form=None,
                    file_weights=None, sample_weights=None, group_metrics=False):
    """Trains `models` surrogates (seeds seed .. seed + models - 1; the pre-shuffle / split uses split_seed, default seed) on the samples of
    `sample_files` and returns a dict: per-model `history` (Keras' loss, mean_absolute_error, val_loss, val_mean_absolute_error per
    epoch), `weights` (models, 104) fp32, `best_model` (lowest final val_loss, ties to the lowest index), `test_metrics` of the best model
    (the notebook's three, scaled space, per output), the scaling tables, the data's time_step_size / dx / dy / dz and the seeds.
    out_dir: also writes the best model's weights.txt, input_scaling.txt, output_scaling.txt and history.json there.
    stencil=True: the two-cell stencil model (9 inputs, `weights` (models, 144), `"inputs": "stencil"` in the result and history.json).
    keep_all=True (with out_dir): also weights_<k>.txt for every trained model, and `surrogate_models` in the result: the list the
    evaluate_surrogates driver takes (names seed<seed>; the scaling files are the shared ones).
    init=DIR (a warm start, e.g. on the old sample files and a rollout's harvested ones together): every model starts from DIR/weights.txt
    instead of its seeded draw -- the models then differ by their epoch shuffles only -- and the scaling tables are DIR's, not the data's
    (samples outside the old range scale outside [0, 1]); the Nadam moments and the step counter start at zero.  The result gains `init`,
    `initial_weights` (models, 104 | 144) and `training_domain` (5 | 9, 2): per input the union of this run's samples' range and DIR's
    training_domain.txt (DIR's input_scaling.txt if DIR has none) -- what the model has now seen, written to out_dir/training_domain.txt
    (`training_domain_file`; with keep_all every `surrogate_models` entry names it as nn_training_domain).  DESIGN.md 13.11.
    form="tendency": the network is fitted to the change of the four fields (labels and output table from after - before; module
    docstring); the result, history.json and the written files carry `form`.  The losses and the test metrics are in scaled LABEL space --
    for a tendency model that is the space of the scaled changes, so they do not compare with a state model's.  form=None: "state", or
    with init=DIR the form of DIR's model; a form that contradicts DIR's is refused (resolve_form).
    file_weights (one float per sample file, in the files' order) or sample_weights ((n,) in concatenated file order; giving both is
    refused): Keras' fit(sample_weight=...) under its default reduction -- the loss of a batch is sum_i w_i mean_o((y - t)^2) / B, the
    divisor the batch size.  The weights are used AS GIVEN, as Keras uses them: no renormalisation, so doubling every weight doubles the
    gradient.  A weight of 0 is allowed (such samples are never trained on; with group_metrics a file of weight 0 is a pure evaluation
    group); non-finite or negative weights, a wrong count, and a training set without a positive weight are refused on the host.  The
    four `history` series are then the weighted quantities (loss = sum w r^2 / (4 n_train), val_loss = sum w d^2 / (4 n_val), the same
    for the two absolute errors) and best_model follows the weighted val_loss; `test_metrics` stay UNWEIGHTED over the whole test set, so
    they compare with any other run.  The result and history.json gain `weighted: True` and `file_weights` (None with sample_weights).
    group_metrics=True (with or without weights) adds `group_metrics`: per file {file, weight, n_train, n_val, n_test, and, unweighted, at
    the best model's final weights: val_loss, val_mean_absolute_error, test_loss and the notebook's three test metrics on that file's
    samples alone}; a file without a sample in a set has None for that set's numbers.  DESIGN.md 13.13."""
    form = resolve_form(form, init)
    inputs, outputs, meta = read_samples(sample_files, stencil=stencil)
    scl_in, scl_out = data_scaling(inputs, outputs, allow_constant=init is not None, form=form)
    n = inputs.shape[0]
    n_split = check_arguments(n, epochs, batch_size, test_split, validation_split, models)
    weights = check_weights(n, meta["file_index"], len(meta["files"]), file_weights, sample_weights)
    check_training_weights(weights, n_split[0], int(seed if split_seed is None else split_seed))
    initial = domain = None
    if init is not None:
        data_in = scl_in
        w0, scl_in, scl_out = load_init(init, stencil)                                 # (refuses the other width before anything else)
        domain = training_domain_union(data_in, init_domain(init, data_in.shape[0]))   # this run's samples and all the model saw before
        initial = np.repeat(w0[None, :], int(models), axis=0)
    import torch
    dev = torch.device(device)
    raw_in = torch.from_numpy(inputs).to(dev)
    raw_out = torch.from_numpy(outputs).to(dev)
    tr = Trainer(raw_in, raw_out, scl_in, scl_out, n_split, seed, split_seed, models, batch_size, epochs, learning_rate, initial=initial, form=form,
                 sample_weights=weights, groups=meta["file_index"] if group_metrics else None)
    if group_metrics:
        tr.n_groups = len(meta["files"])                                      # (a last file without samples is a group too)
    if verbose:
        print("output form: %s -- loss, errors and test metrics below are in scaled label space: %s"
              % (form, "the scaled change (after - before) of each field" if form == "tendency" else "the scaled new value of each field"), flush=True)
    del raw_in, raw_out
    K, (n_train, n_val, n_test) = int(models), n_split
    hist = [{"loss": [], "mean_absolute_error": [], "val_loss": [], "val_mean_absolute_error": []} for _ in range(K)]
    secs = []

    def add_val(vs):
        for m in range(K):
            s = vs[m].reshape(4, 6)
            hist[m]["val_loss"].append(float(s[:, 0].sum() / (4 * n_val)))
            hist[m]["val_mean_absolute_error"].append(float(s[:, 1].sum() / (4 * n_val)))

    def report(e):
        if not verbose:
            return
        print("Epoch %d/%d" % (e + 1, epochs))
        for m in range(K):
            h = hist[m]
            print("%s%d/%d - %.3fs - loss: %.4e - mean_absolute_error: %.4e - val_loss: %.4e - val_mean_absolute_error: %.4e"
                  % ("model %d: " % m if K > 1 else "", tr.steps, tr.steps, secs[e], h["loss"][e], h["mean_absolute_error"][e],
                     h["val_loss"][e], h["val_mean_absolute_error"][e]), flush=True)

    t0 = time.perf_counter()
    for e in range(int(epochs)):
        w, ts, vs = tr.epoch()
        secs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for m in range(K):
            hist[m]["loss"].append(float(ts[m, 0] / (4 * n_train)))
            hist[m]["mean_absolute_error"].append(float(ts[m, 1] / (4 * n_train)))
        if e > 0:
            add_val(vs)
            report(e - 1)
    w, _, vs = tr.finish()
    add_val(vs)
    report(int(epochs) - 1)
    final = np.array([h["val_loss"][-1] for h in hist])
    best = int(np.argmin(final))                                        # first minimum: ties go to the lowest index
    tst = tr.test_errors(w[best])
    metrics = _metrics(tst)
    metrics["test_loss"] = float(tst[:, 0].sum() / (4 * n_test))
    seeds = [int(seed) + m for m in range(K)]
    result = {"history": hist, "weights": w, "best_model": best, "test_metrics": metrics, "input_scaling": scl_in, "output_scaling": scl_out,
              "seeds": seeds, "split_seed": tr.split_seed, "n_train": n_train, "n_val": n_val, "n_test": n_test, "epoch_seconds": secs,
              "batch_size": int(batch_size), "epochs": int(epochs), "learning_rate": float(learning_rate),
              "inputs": "stencil" if stencil else "single_cell", "form": form}
    result.update({k: meta[k] for k in ("time_step_size", "dx", "dy", "dz", "files")})
    if init is not None:
        result["init"], result["initial_weights"], result["training_domain"] = os.fspath(init), initial, domain
    if weights is not None:
        result["weighted"], result["file_weights"] = True, None if file_weights is None else [float(v) for v in file_weights]
    if verbose:
        print("Max relative errors:  ", metrics["max_relative_error"])
        print("Mean relative errors: ", metrics["mean_relative_error"])
        print("Mean relative bias:   ", metrics["mean_relative_bias"], flush=True)
    if group_metrics:
        result["group_metrics"] = _group_records(tr, w[best], meta["files"], file_weights, unweighted=weights is None)
        if verbose:
            for g in result["group_metrics"]:
                print(group_line(g), flush=True)
    if out_dir is not None:
        js = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in result.items() if k != "weights"}
        js["best_weights"] = w[best].astype(np.float64).tolist()
        if keep_all:
            result["files_written"], result["surrogate_models"] = write_outputs(out_dir, w[best], scl_in, scl_out, js, all_weights=w,
                                                                                    names=["seed%d" % sd for sd in seeds], form=form)
        else:
            result["files_written"] = write_outputs(out_dir, w[best], scl_in, scl_out, js, form=form)
        if domain is not None:                                               # the scaling rows stay DIR's; the domain follows the samples
            result["training_domain_file"] = write_training_domain(out_dir, domain)
            for m in result.get("surrogate_models", ()):
                m["nn_training_domain"] = result["training_domain_file"]
    return result


def committee_snippet(names, name="committee"):
    """The `surrogate_committees:` lines that make one committee of the named models (the drivers' committee_config reads them)."""
    if len(names) > 16:
        raise SurrogateTrainError("--committee: %d models were trained, a committee holds at most 16" % len(names))
    return "surrogate_committees:\n  - {name: %s, members: [%s]}" % (name, ", ".join(names))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m miniweatherml_amd.surrogate_train",
                                 description="Train the Kessler surrogate (5 -> 10 -> 4, or 9 -> 10 -> 4 with --stencil) on DataGenerator sample files, on the GPU.")
    ap.add_argument("files", nargs="+", help="sample files written by generate_micro_data (concatenated in this order)")
    ap.add_argument("--out", required=True, help="directory for weights.txt, input_scaling.txt, output_scaling.txt, history.json")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--test-split", type=float, default=0.2)
    ap.add_argument("--validation-split", type=float, default=0.2)
    ap.add_argument("--learning-rate", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--split-seed", type=int, default=None, help="seed of the pre-shuffle (default: --seed)")
    ap.add_argument("--models", type=int, default=1, help="train seeds seed .. seed+K-1 at once and keep the best (lowest val_loss)")
    ap.add_argument("--keep-all", action="store_true", help="also write weights_<k>.txt for every trained model and print the surrogate_models list "
                    "for the evaluate_surrogates and rollout_surrogates drivers")
    ap.add_argument("--committee", action="store_true", help="with --keep-all: also print a surrogate_committees list that names all trained models "
                    "(at most 16 form a committee)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--init", default=None, metavar="DIR", help="warm start: continue DIR/weights.txt with DIR's scaling tables (all models start there)")
    ap.add_argument("--stencil", action="store_true", help="train the two-cell stencil model (the cell and the level above: 9 inputs, 144 weights)")
    ap.add_argument("--tendency", action="store_true", help="train the tendency form: the network predicts the change of the four fields, which inference "
                    "adds to the state in fp64 (with --init DIR the form is DIR's; a state-form DIR is refused)")
    ap.add_argument("--file-weights", default=None, metavar="W,W,...", help="one weight per sample file, in their order (Keras' sample_weight: the "
                    "batch loss is sum w (y - t)^2 / batch size, weights as given; 0 = evaluate the file only)")
    ap.add_argument("--group-metrics", action="store_true", help="also report validation and test errors of every sample file on its own")
    a = ap.parse_args(argv)
    try:
        r = train_surrogate(a.files, a.out, a.epochs, a.batch_size, a.test_split, a.validation_split, a.learning_rate, a.seed, a.models,
                            a.device, a.split_seed, verbose=True, stencil=a.stencil, keep_all=a.keep_all,
                            init=a.init, form="tendency" if a.tendency else None,
                            file_weights=None if a.file_weights is None else parse_file_weights(a.file_weights), group_metrics=a.group_metrics)
    except SurrogateTrainError as e:
        print("ERROR: %s" % e, file=sys.stderr)
        return 2
    print("best model %d (seed %d); wrote %s" % (r["best_model"], r["seeds"][r["best_model"]], ", ".join(r["files_written"])))
    if a.keep_all:
        print("surrogate_models:")
        for m in r["surrogate_models"]:
            print("  - {%s}" % ", ".join("%s: %s" % kv for kv in m.items()))
        if a.committee:
            print(committee_snippet([m["name"] for m in r["surrogate_models"]]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
