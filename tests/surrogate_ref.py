"""Yardsticks of the surrogate trainer (csrc/mw_train.hip, miniweatherml_amd/surrogate_train.py), written from the algorithm's definition:
the prepare step on the host, the batch gradient as per-sample fp64 contributions (and two fp32 evaluations of the same gradient to measure
what fp32 itself costs), the error sums of a prediction in extended precision, and ONE torch replay of a training run in the product's batch
order.  A plain module (no fixtures): tests/test_surrogate_ref_cpu.py checks it on the CPU, the GPU tests compare the kernels with it."""
import math

import numpy as np

U32 = 2.0 ** -24                                                       # unit roundoff of fp32
U64 = 2.0 ** -53
_LONG = np.finfo(np.longdouble).nmant >= 63                             # x87 extended precision; else the sums fall back to math.fsum

GRAD_BATCHES = (1, 2, 3, 63, 64, 65, 127, 255, 256, 257, 300, 1024, 4097, 8191, 8192)
NEAR_FIT_BATCHES = (300, 1024, 8192)
PREPARE_SIZES = (3, 4, 5, 16, 17, 255, 256, 257, 65536, 65537, 4096 * 256 + 777)
SPLITS = ((0.2, 0.2), (0.5, 0.1))                                       # (test_split, validation_split): the notebook's, one uneven
ERROR_SIZES = (1, 2, 255, 256, 257, 128 * 256 - 1, 128 * 256, 128 * 256 + 1, 1000003)
ERROR_NSETS = (1, 2, 3, 5)


def n_par(n_in):
    return 10 * n_in + 54


# ---------------------------------------------------------------------------------------------------------------------------------
# the prepare step
def host_sets(inputs, outputs, split_seed, test_split=0.2, validation_split=0.2):
    """The device's prepare step restated: pre-shuffle, min-max scaling in fp64 rounded to fp32, [train | val | test]."""
    from miniweatherml_amd import surrogate_train as st
    n = inputs.shape[0]
    perm = st.preshuffle_permutation(n, split_seed)
    lo_i, hi_i, lo_o, hi_o = inputs.min(0), inputs.max(0), outputs.min(0), outputs.max(0)
    xs = ((inputs[perm].astype(np.float64) - lo_i) / (hi_i.astype(np.float64) - lo_i)).astype(np.float32)
    ys = ((outputs[perm].astype(np.float64) - lo_o) / (hi_o.astype(np.float64) - lo_o)).astype(np.float32)
    n_train, n_val, _ = st.split_sizes(n, test_split, validation_split)
    cut = [0, n_train, n_train + n_val, n]
    return [(xs[cut[k]:cut[k + 1]], ys[cut[k]:cut[k + 1]]) for k in range(3)]


def prepare_cases():
    """(n, test_split, validation_split) of tests/test_gpu_surrogate_trainer.py: every size with the notebook's split, and with the uneven
    one wherever all three sets stay non-empty."""
    from miniweatherml_amd import surrogate_train as st
    return [(n, ts, vs) for n in PREPARE_SIZES for ts, vs in SPLITS if min(st.split_sizes(n, ts, vs)) >= 1]


def raw_samples(n, n_in, seed):
    """Raw fp32 samples (n, n_in), (n, 4) with Kessler-like magnitudes (each variable its own offset and range)."""
    rng = np.random.default_rng(seed)
    lo = np.array([200.0, 0.1, 0.0, 1e-5, -3.0, 195.0, 0.0, 2.0, 1e3])[:n_in]
    rg = np.array([100.0, 1.1, 0.02, 0.004, 7.0, 100.0, 0.018, 0.004, 5e4])[:n_in]
    x = (lo + rg * rng.random((n, n_in))).astype(np.float32)
    y = (np.array([250.0, 0.0, -1e-3, 10.0]) + np.array([60.0, 0.02, 5e-3, 1e-2]) * rng.random((n, 4))).astype(np.float32)
    return x, y


# ---------------------------------------------------------------------------------------------------------------------------------
# the batch gradient
def gradient_case(n_in, batch):
    """The batch of the gradient tests, seeded by its size: weights N(0, 0.6) with the hidden biases shifted by -0.5 (pre-activations of
    both signs), x (n_in, batch) and y (4, batch) uniform in [0, 1), all fp32, feature-major as the kernel takes them."""
    rng = np.random.default_rng(batch)
    w = (rng.standard_normal(n_par(n_in)) * 0.6).astype(np.float32)
    w[10 * n_in:10 * n_in + 10] -= 0.5
    x = rng.random((n_in, batch), dtype=np.float32)
    y = rng.random((4, batch), dtype=np.float32)
    return w, x, y


def forward64(w, x):
    """The network in fp64 on sample-major x (B, n_in): (pre-activations (B, 10), outputs (B, 4))."""
    from miniweatherml_amd import surrogate_train as st
    W1, b1, W2, b2 = [np.asarray(a, np.float64) for a in st.split_weights(w)]
    pre = np.asarray(x, np.float64) @ W1 + b1
    return pre, np.where(pre > 0, pre, 0.1 * pre) @ W2 + b2


def near_fit_case(n_in, batch):
    """gradient_case with targets next to the network's own output: y = fp64 forward + 1e-2 N(0, 1).  The residuals are centred, so every
    gradient entry is a sum that cancels."""
    w, x, _ = gradient_case(n_in, batch)
    out = forward64(w, x.T)[1]
    y = out + 1e-2 * np.random.default_rng(1000 + batch).standard_normal(out.shape)
    return w, x, np.ascontiguousarray(y.T.astype(np.float32))


def signs_ok(n_in, w, x):
    """The gradient tests' precondition: both branches of the leaky ReLU are taken -- at least one pre-activation of each sign below one
    wave, at least 5 % of each from there on."""
    pre = forward64(w, x.T)[0]
    pos, neg = float((pre > 0).mean()), float((pre < 0).mean())
    return (pos > 0 and neg > 0) if x.shape[1] < 64 else (pos >= 0.05 and neg >= 0.05)


def _terms(n_in, w, x, y, dtype):
    """Per-sample contributions in `dtype`, one rounding per operation, sums in index order."""
    a = 10 * n_in
    w, x, y = [np.asarray(v, dtype) for v in (w, x, y)]
    W1, b1, W2, b2 = w[:a].reshape(n_in, 10), w[a:a + 10], w[a + 10:a + 50].reshape(10, 4), w[a + 50:]
    B = x.shape[0]
    pre = np.empty((B, 10), dtype)
    for u in range(10):
        acc = np.zeros(B, dtype)
        for i in range(n_in):
            acc = acc + x[:, i] * W1[i, u]
        pre[:, u] = acc + b1[u]
    pos = pre > 0
    h = np.where(pos, pre, dtype(0.1) * pre)
    r = np.empty((B, 4), dtype)
    for o in range(4):
        acc = np.zeros(B, dtype)
        for u in range(10):
            acc = acc + h[:, u] * W2[u, o]
        r[:, o] = (acc + b2[o]) - y[:, o]
    dpre = np.empty((B, 10), dtype)
    for u in range(10):
        acc = np.zeros(B, dtype)
        for o in range(4):
            acc = acc + r[:, o] * W2[u, o]
        dpre[:, u] = np.where(pos[:, u], acc, dtype(0.1) * acc)
    terms = np.empty((B, n_par(n_in)), dtype)
    terms[:, :a] = (x[:, :, None] * dpre[:, None, :]).reshape(B, a)
    terms[:, a:a + 10] = dpre
    terms[:, a + 10:a + 50] = (h[:, :, None] * r[:, None, :]).reshape(B, 40)
    terms[:, a + 50:] = r
    assert terms.dtype == dtype
    return terms


def grad_terms(n_in, w, x, y):
    """terms[B, npar] in fp64: sample s's contribution to every parameter's gradient of sum_o (out_o - y_o)^2 / 2, in the product's
    parameter order W1 (n_in, 10), b1, W2 (10, 4), b2.  x (B, n_in), y (B, 4) sample-major.  With r = out - y, delta = leaky'(pre) * (W2 r):
    W1[i, u]: x_i delta_u;  b1[u]: delta_u;  W2[u, o]: h_u r_o;  b2[o]: r_o.  The gradient of mean((out - y)^2) is their sum times
    2 / (4 B) (grad_summary)."""
    return _terms(n_in, w, x, y, np.float64)


def grad_summary(terms):
    """(g_ref, T, loss, mean|r|) of a batch from its terms: g_ref = sum * 0.5 / B, T = the same sum of absolute values (the size of what
    is added up for that entry), and -- the last four columns being r itself -- loss = mean r^2 and mean |r|."""
    B = terms.shape[0]
    r = terms[:, -4:]
    return terms.sum(0) * 0.5 / B, np.abs(terms).sum(0) * 0.5 / B, float(np.sum(r * r) / (4 * B)), float(np.abs(r).sum() / (4 * B))


def rho(g, g_ref, T):
    """max_e |g - g_ref|_e / (2^-24 T_e): the error of each entry in units of ONE fp32 rounding of that entry's own sum."""
    return float(np.max(np.abs(np.asarray(g, np.float64) - g_ref) / (U32 * T)))


def grad_fp32_torch(n_in, w, x, y):
    """(gradient, loss) by torch fp32 autograd on the CPU."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    P = [torch.tensor(np.array(a, np.float32)).requires_grad_() for a in st.split_weights(np.asarray(w, np.float32))]
    loss = torch.nn.functional.mse_loss(torch_forward(P, torch.tensor(np.array(x, np.float32))), torch.tensor(np.array(y, np.float32)))
    loss.backward()
    return np.concatenate([p.grad.numpy().ravel() for p in P]).astype(np.float64), float(loss.detach())


def grad_fp32_index_order(n_in, w, x, y):
    """The gradient from fp32 per-sample terms added one after the other in index order."""
    t = _terms(n_in, w, x, y, np.float32)
    s = np.cumsum(t, axis=0, dtype=np.float32)[-1]
    return (s * np.float32(0.5 / t.shape[0])).astype(np.float64)


def fp32_rho(n_in, w, x, y, g_ref, T):
    """max of the two fp32 evaluations' rho: what plain fp32 costs on this batch."""
    return max(rho(grad_fp32_torch(n_in, w, x, y)[0], g_ref, T), rho(grad_fp32_index_order(n_in, w, x, y), g_ref, T))


def device_batch_grad(n_in, w, x, y, v2=True):
    """mw_surrogate_batch_grad_v2 (v2=False: the single-cell entry mw_surrogate_batch_grad) on feature-major fp32 x (n_in, B), y (4, B):
    (gradient as fp64, loss)."""
    import ctypes
    import torch
    from miniweatherml_amd import capi
    B = x.shape[1]
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (w, x, y)]
    grad = torch.full((n_par(n_in),), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in dev + [grad, loss]]
    if v2:
        capi.check(capi.lib().mw_surrogate_batch_grad_v2(n_in, ptr[0], ptr[1], ptr[2], B, ptr[3], ptr[4], None))
    else:
        assert n_in == 5
        capi.check(capi.lib().mw_surrogate_batch_grad(ptr[0], ptr[1], ptr[2], B, ptr[3], ptr[4], None))
    torch.cuda.synchronize()
    return grad.cpu().numpy().astype(np.float64), float(loss.cpu()[0])


def check_rho(n_in, w, x, y, g, what):
    """Prints and asserts rho(device) <= 4 max(rho(torch fp32), rho(fp32 index order)) on the same batch; returns (rho, right-hand side / 4).
    The factor 4: the kernel's order (4-sample MFMA steps, then waves 0..3) is neither of the two, and rho is a maximum over ~100 roundings."""
    g_ref, T, _, _ = grad_summary(grad_terms(n_in, w, x.T, y.T))
    got, cpu = rho(g, g_ref, T), fp32_rho(n_in, w, x.T, y.T, g_ref, T)
    print("%s: rho(kernel) %.1f, rho(fp32 on the CPU) %.1f, max|dg|/max|g| %.2e" % (what, got, cpu, np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref))))
    assert got <= 4.0 * cpu, (what, got, cpu)
    return got, cpu


# ---------------------------------------------------------------------------------------------------------------------------------
# the error sums
def _sum(a):
    a = np.asarray(a, np.float64).ravel()
    return float(np.sum(a.astype(np.longdouble))) if _LONG else math.fsum(a.tolist())


def error_sums_ref(pred, y):
    """k_surrogate_sums' statistics of one set: pred, y (4, n) -> (stats (4, 6) = [sum d^2, sum |d|, sum d, sum |t|, max |d|, max |t|] per
    output, with d = t - pred in fp64; mass (4, 4) = the sum of ABSOLUTE values of what each of the four sums adds, for the bound
    n 2^-52 mass of an n-term fp64 sum in any order).  The sums are taken in extended precision, the maxima are exact."""
    pred, y = np.asarray(pred, np.float64), np.asarray(y, np.float64)
    stats, mass = np.zeros((4, 6)), np.zeros((4, 4))
    for o in range(4):
        t = y[o]
        d = t - pred[o]
        sq = _sum(d * d) if not _LONG else float(np.sum(d.astype(np.longdouble) ** 2))
        stats[o] = [sq, _sum(np.abs(d)), _sum(d), _sum(np.abs(t)), np.max(np.abs(d)), np.max(np.abs(t))]
        mass[o] = [stats[o, 0], stats[o, 1], stats[o, 1], stats[o, 3]]
    return stats, mass


def errors_case(n, nsets, seed=0):
    """pred (nsets, 4, n), y (4, n) fp32 for the error-sum tests: signed differences; output 0's targets all negative (|t| matters);
    output 1 with one outlier of t and of d at the LAST index; every set its own predictions."""
    rng = np.random.default_rng([n, nsets, seed])
    y = rng.standard_normal((4, n)).astype(np.float32)
    y[0] = -np.abs(y[0]) - np.float32(0.25)
    pred = (y[None] + 0.3 * rng.standard_normal((nsets, 4, n))).astype(np.float32)
    y[1, n - 1] = 1000.0
    pred[:, 1, n - 1] = np.float32(-500.0) - np.arange(nsets, dtype=np.float32)
    return np.ascontiguousarray(pred), np.ascontiguousarray(y)


def metrics_of(stats, n):
    """The trainer's report from one set's statistics: the notebook's three metrics per output, and the loss."""
    s = np.asarray(stats, np.float64).reshape(4, 6)
    return {"max_relative_error": s[:, 4] / s[:, 5], "mean_relative_error": s[:, 1] / s[:, 3], "mean_relative_bias": s[:, 2] / s[:, 3],
            "test_loss": float(s[:, 0].sum() / (4 * n))}


def check_test_metrics(result, test_set, what=""):
    """result = train_surrogate's dict, test_set = host_sets' third pair.  Reference: the best model's final weights through the fp64
    forward on the test split, error_sums_ref.  The product predicts with the MFMA forward, which the suite holds to 1e-5 on the scaled
    outputs; a shift of every prediction by at most 1e-5 moves the two mean metrics by at most 1e-5 / mean|t|, the max metric by
    1e-5 / max|t| and the loss by 2e-5 mean|d| (+ 1e-10 for its square)."""
    sx, sy = test_set
    n = sx.shape[0]
    assert n == result["n_test"]
    out = forward64(result["weights"][result["best_model"]], sx)[1]
    stats, _ = error_sums_ref(out.T, sy.T)
    ref, tm = metrics_of(stats, n), result["test_metrics"]
    mean_t, max_t, mean_d = stats[:, 3] / n, stats[:, 5], stats[:, 1].sum() / (4 * n)
    tol = {"max_relative_error": 1e-5 / max_t, "mean_relative_error": 1e-5 / mean_t, "mean_relative_bias": 1e-5 / mean_t}
    for key in tol:
        err = np.abs(np.asarray(tm[key]) - ref[key])
        print("%s %-20s %s  (reference %s, |diff| / tolerance %s)" % (what, key, np.array2string(np.asarray(tm[key]), precision=5),
              np.array2string(ref[key], precision=5), np.array2string(err / tol[key], precision=2)))
        assert np.all(err <= tol[key]), (what, key, err / tol[key])
    err = abs(tm["test_loss"] - ref["test_loss"])
    print("%s test_loss %.6e (reference %.6e, |diff| / tolerance %.2g)" % (what, tm["test_loss"], ref["test_loss"], err / (2e-5 * mean_d + 1e-10)))
    assert err <= 2e-5 * mean_d + 1e-10, (what, err, 2e-5 * mean_d + 1e-10)
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
# the training run
# the edge configurations of tests/test_gpu_surrogate_trainer.py: samples, batch size, epochs, learning rate, (n_train, n_val, n_test), steps
CONFIGS = {"a": dict(n=400, batch=1, epochs=1, lr=1e-3, split=(256, 64, 80), steps=256),          # 256 steps with one live lane
           "b": dict(n=1000, batch=1024, epochs=2, lr=1e-3, split=(640, 160, 200), steps=1),       # the training set is smaller than a batch
           "c": dict(n=20000, batch=8192, epochs=2, lr=1e-3, split=(12800, 3200, 4000), steps=2),  # 8192 + 4608
           "d": dict(n=5000, batch=100, epochs=2, lr=1e-3, split=(3200, 800, 1000), steps=32),     # no partial batch: the prefetch ends
           "e": dict(n=20000, batch=257, epochs=2, lr=1e-2, split=(12800, 3200, 4000), steps=50)}
CONFIG_CASES = [(c, False) for c in "abcde"] + [(c, True) for c in "acd"]                         # (configuration, stencil)
CONFIG_SEED = 7


def torch_model(w, dtype=None):
    import torch
    from miniweatherml_amd import surrogate_train as st
    dtype = dtype or torch.float64
    return [torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype).clone().requires_grad_() for a in st.split_weights(w)]


def torch_forward(P, x):
    import torch
    return torch.nn.functional.leaky_relu(x @ P[0] + P[1], 0.1) @ P[2] + P[3]


SERIES = ("loss", "mean_absolute_error", "val_loss", "val_mean_absolute_error")


def replay(dtype, sets, seed, batch, epochs, lr=1e-3, stencil=False, model=0):
    """A training run of model `model` in torch `dtype` (Linear -> leaky_relu(0.1) -> Linear, mse_loss, NAdam(eps=1e-7, momentum_decay=4e-3))
    from the product's seeded initial weights in the product's batch order, on host_sets' sets.  Returns (weights as fp64, history): per
    epoch Keras' running `loss` and `mean_absolute_error` (each batch with the weights it was trained at) and the validation set's after
    the epoch."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    (tx, ty), (vx, vy) = sets[0], sets[1]
    assert tx.shape[1] == (9 if stencil else 5)
    P = torch_model(st.initial_weights(seed + model, 1, stencil=stencil)[0], dtype)
    opt = torch.optim.NAdam(P, lr=lr, betas=(0.9, 0.999), eps=1e-7, momentum_decay=4e-3)
    X, Y, VX, VY = [torch.tensor(a.astype(np.float64)).to(dtype) for a in (tx, ty, vx, vy)]
    hist = {k: [] for k in SERIES}
    for e in range(epochs):
        order = torch.from_numpy(st.epoch_permutation(len(tx), seed, model, e))
        tot, tot_abs = 0.0, 0.0
        for s in range(0, len(tx), batch):
            idx = order[s:s + batch]
            opt.zero_grad()
            out = torch_forward(P, X[idx])
            loss = torch.nn.functional.mse_loss(out, Y[idx])
            loss.backward()
            opt.step()
            tot += float(loss.detach()) * len(idx)
            tot_abs += float((out.detach() - Y[idx]).abs().mean()) * len(idx)
        hist["loss"].append(tot / len(tx))
        hist["mean_absolute_error"].append(tot_abs / len(tx))
        with torch.no_grad():
            vout = torch_forward(P, VX)
            hist["val_loss"].append(float(torch.nn.functional.mse_loss(vout, VY)))
            hist["val_mean_absolute_error"].append(float((vout - VY).abs().mean()))
    return np.concatenate([p.detach().numpy().ravel() for p in P]).astype(np.float64), hist


def deviations(weights, history, w_ref, hist_ref):
    """(max|dw| / max|w|, then the largest relative deviation of each of the four series) of a run against a replay."""
    w = np.asarray(weights, np.float64)
    out = [float(np.max(np.abs(w - w_ref)) / np.max(np.abs(w_ref)))]
    for k in SERIES:
        assert len(history[k]) == len(hist_ref[k])
        out.append(max(abs(a - b) / b for a, b in zip(history[k], hist_ref[k])))
    return tuple(out)


def emulate_trainer(sets, seed, batch, epochs, table, stencil=False):
    """The kernel's update on the CPU: exact (fp64) batch gradients rounded to fp32, then k_surrogate_train's fp32 Nadam expressions with
    the per-step scalars of `table` and beta1, beta2, eps as the kernel receives them (fp32).  What is left against the fp64 replay is the
    update's own error."""
    from miniweatherml_amd import surrogate_train as st
    f32 = np.float32
    tx, ty = sets[0]
    w = st.initial_weights(seed, 1, stencil=stencil)[0].copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    b1, b2, eps = f32(st.NADAM["beta1"]), f32(st.NADAM["beta2"]), f32(st.NADAM["eps"])
    k = 0
    for e in range(epochs):
        order = st.epoch_permutation(len(tx), seed, 0, e)
        for s in range(0, len(tx), batch):
            idx = order[s:s + batch]
            gr = grad_summary(grad_terms(tx.shape[1], w, tx[idx], ty[idx]))[0].astype(f32)
            cg, cm, bc2 = table[k]
            k += 1
            m = b1 * m + (f32(1) - b1) * gr
            v = b2 * v + (f32(1) - b2) * gr * gr
            w = w - (cg * gr + cm * m) / (np.sqrt(v / bc2) + eps)
            assert w.dtype == f32
    return w.astype(np.float64)
