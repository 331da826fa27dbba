"""Yardsticks of weighted surrogate training (mw_surrogate_*_w, mw_surrogate_errors_weighted, mw_surrogate_prepare_column; DESIGN.md
section 13.13), written from Keras' definition of sample_weight on top of tests/surrogate_ref.py, which this module imports and leaves as
it is: the weighted batch gradient as per-sample fp64 terms (and its two fp32 evaluations), the weighted error sums, ONE weighted torch
replay of a training run, the split of a per-sample column, and the two sample files of the end-to-end tests.  A plain module (no
fixtures): tests/test_surrogate_weighted_cpu.py checks it on the CPU, tests/test_gpu_surrogate_weighted.py compares the kernels with it."""
import numpy as np

import surrogate_ref as sr

PLANTED = (0, 63, 64, 255, 256)                                          # lane 63 / 64, chunk position 255 / 256 (and B - 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# weights
def log_uniform_weights(n, seed):
    """(n,) fp32, log-uniform in [2^-4, 2^4]."""
    return np.exp2(np.random.default_rng([n, seed]).uniform(-4.0, 4.0, n)).astype(np.float32)


def planted_weights(n):
    """(n,) fp32: ones, with 16s and zeros alternating at the positions PLANTED and n - 1 where they exist (the first is a 16, so that a
    batch of one sample keeps a gradient)."""
    w = np.ones(n, np.float32)
    for k, p in enumerate(sorted({q for q in PLANTED + (n - 1,) if 0 <= q < n})):
        w[p] = 16.0 if k % 2 == 0 else 0.0
    return w


# ---------------------------------------------------------------------------------------------------------------------------------
# the weighted batch gradient
def weighted_terms(n_in, w, x, y, wt, dtype=np.float64):
    """surrogate_ref._terms scaled per sample: sample s's contribution to the gradient of sum_s wt_s sum_o (out - y)^2 / 2."""
    return sr._terms(n_in, w, x, y, dtype) * np.asarray(wt, dtype)[:, None]


def weighted_summary(n_in, w, x, y, wt):
    """(g_ref, T, loss, mae) of the weighted batch in fp64: g_ref = sum of the weighted terms * 0.5 / B, T the same sum of their absolute
    values (the rho yardstick's unit), loss = sum w r^2 / (4 B), mae = sum w |r| / (4 B).  x (B, n_in), y (B, 4) sample-major."""
    t = weighted_terms(n_in, w, x, y, wt)
    B = t.shape[0]
    r = sr._terms(n_in, w, x, y, np.float64)[:, -4:]
    w64 = np.asarray(wt, np.float64)[:, None]
    return t.sum(0) * 0.5 / B, np.abs(t).sum(0) * 0.5 / B, float(np.sum(w64 * r * r) / (4 * B)), float(np.sum(w64 * np.abs(r)) / (4 * B))


def grad_fp32_torch(n_in, w, x, y, wt):
    """(gradient, loss) of the weighted batch by torch fp32 autograd on the CPU: loss = mean(wt[:, None] (out - y)^2)."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    P = [torch.tensor(np.array(a, np.float32)).requires_grad_() for a in st.split_weights(np.asarray(w, np.float32))]
    out = sr.torch_forward(P, torch.tensor(np.array(x, np.float32)))
    loss = (torch.tensor(np.array(wt, np.float32))[:, None] * (out - torch.tensor(np.array(y, np.float32))) ** 2).mean()
    loss.backward()
    return np.concatenate([p.grad.numpy().ravel() for p in P]).astype(np.float64), float(loss.detach())


def grad_fp32_index_order(n_in, w, x, y, wt):
    """The weighted gradient from fp32 per-sample terms added one after the other in index order."""
    t = weighted_terms(n_in, w, x, y, wt, np.float32)
    assert t.dtype == np.float32
    return (np.cumsum(t, axis=0, dtype=np.float32)[-1] * np.float32(0.5 / t.shape[0])).astype(np.float64)


def fp32_rho(n_in, w, x, y, wt, g_ref, T):
    """max of the two fp32 evaluations' rho on the same weighted batch (surrogate_ref.fp32_rho's)."""
    return max(sr.rho(grad_fp32_torch(n_in, w, x, y, wt)[0], g_ref, T), sr.rho(grad_fp32_index_order(n_in, w, x, y, wt), g_ref, T))


def device_batch_grad_w(n_in, w, x, y, wt):
    """mw_surrogate_batch_grad_w on feature-major fp32 x (n_in, B), y (4, B), wt (B,): (gradient fp32, loss fp32) as numpy."""
    import ctypes
    import torch
    from miniweatherml_amd import capi
    B = x.shape[1]
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (w, x, y, wt)]
    grad = torch.full((sr.n_par(n_in),), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in dev + [grad, loss]]
    capi.check(capi.lib().mw_surrogate_batch_grad_w(n_in, ptr[0], ptr[1], ptr[2], ptr[3], B, ptr[4], ptr[5], None))
    torch.cuda.synchronize()
    return grad.cpu().numpy(), loss.cpu().numpy()[0]


def device_batch_grad_v2(n_in, w, x, y):
    """mw_surrogate_batch_grad_v2, the results kept in fp32 (for bit comparisons)."""
    import ctypes
    import torch
    from miniweatherml_amd import capi
    B = x.shape[1]
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (w, x, y)]
    grad = torch.full((sr.n_par(n_in),), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in dev + [grad, loss]]
    capi.check(capi.lib().mw_surrogate_batch_grad_v2(n_in, ptr[0], ptr[1], ptr[2], B, ptr[3], ptr[4], None))
    torch.cuda.synchronize()
    return grad.cpu().numpy(), loss.cpu().numpy()[0]


def check_rho(n_in, w, x, y, wt, g, what):
    """surrogate_ref.check_rho for a weighted batch: rho(device) <= 4 max(rho(torch fp32), rho(fp32 index order)), all three against the
    fp64 weighted terms; the factor 4 is the project's (surrogate_ref.check_rho).  x (n_in, B), y (4, B) feature-major."""
    g_ref, T, _, _ = weighted_summary(n_in, w, x.T, y.T, wt)
    live = T > 0                                                         # (an entry whose every term is zero: only with all weights zero)
    assert live.all()
    got, cpu = sr.rho(g, g_ref, T), fp32_rho(n_in, w, x.T, y.T, wt, g_ref, T)
    print("%s: rho(kernel) %.1f, rho(fp32 on the CPU) %.1f" % (what, got, cpu))
    assert got <= 4.0 * cpu, (what, got, cpu)
    return got, cpu


# ---------------------------------------------------------------------------------------------------------------------------------
# the weighted error sums
def error_sums_ref(pred, y, wt):
    """k_surrogate_sums<weighted>'s statistics of one set: pred, y (4, n), wt (n,) -> (stats (4, 6), mass (4, 4)) as
    surrogate_ref.error_sums_ref gives them.  The terms are the fp64 numbers d (d w), w |d|, w d, w |t| (the weight applied to d first:
    a weight of 1 leaves every term as it was), summed with surrogate_ref._sum; the maxima over the samples with w > 0 (0 without one)."""
    pred, y, w = np.asarray(pred, np.float64), np.asarray(y, np.float64), np.asarray(wt, np.float64)
    stats, mass = np.zeros((4, 6)), np.zeros((4, 4))
    on = w > 0
    for o in range(4):
        t = y[o]
        d = t - pred[o]
        sq, ab = d * (d * w), w * np.abs(d)
        stats[o] = [sr._sum(sq), sr._sum(ab), sr._sum(w * d), sr._sum(w * np.abs(t)), np.max(np.abs(d[on]), initial=0.0),
                    np.max(np.abs(t[on]), initial=0.0)]
        mass[o] = [sr._sum(np.abs(sq)), sr._sum(ab), sr._sum(ab), sr._sum(w * np.abs(t))]
    return stats, mass


def device_errors(pred, y, wt=None):
    """mw_surrogate_errors_weighted (wt None: mw_surrogate_errors) on pred (nsets, 4, n), y (4, n), wt (n,) fp32: (nsets, 4, 6) fp64."""
    import ctypes
    import torch
    from miniweatherml_amd import capi
    nsets, _, n = pred.shape
    L = capi.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                        # noqa: E731
    dp, dy = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()
    ws = torch.empty(int(L.mw_surrogate_errors_workspace_bytes(nsets)), dtype=torch.uint8, device="cuda")
    out = torch.full((nsets, 24), float("nan"), dtype=torch.float64, device="cuda")
    if wt is None:
        capi.check(L.mw_surrogate_errors(n, nsets, ptr(dp), ptr(dy), ptr(ws), ptr(out), None))
    else:
        dw = torch.from_numpy(np.ascontiguousarray(wt, np.float32)).cuda()
        capi.check(L.mw_surrogate_errors_weighted(n, nsets, ptr(dp), ptr(dy), ptr(dw), ptr(ws), ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nsets, 4, 6)


# ---------------------------------------------------------------------------------------------------------------------------------
# the column split
def split_column(col, seed, n_train, n_val):
    """mw_surrogate_prepare_column on the host: col[perm][:n_train], [n_train:n_train + n_val], the rest."""
    from miniweatherml_amd import surrogate_train as st
    c = np.asarray(col)[st.preshuffle_permutation(len(col), seed)]
    return c[:n_train], c[n_train:n_train + n_val], c[n_train + n_val:]


# ---------------------------------------------------------------------------------------------------------------------------------
# the weighted training run
def replay(dtype, sets, wsets, seed, batch, epochs, lr=1e-3, stencil=False, model=0, initial=None):
    """surrogate_ref.replay with Keras' sample_weight: the loss of a batch is (w[idx, None] * (out - Y[idx]) ** 2).mean(), the same
    NAdam(eps=1e-7, momentum_decay=4e-3), the product's batch order.  sets: host_sets' sets; wsets: (train weights, validation weights).
    The four series are the weighted ones (loss = sum w r^2 / (4 n_train), ...), the validation set weighted with its own weights.
    initial: the starting weights of a continued model instead of the seeded draw."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    (tx, ty), (vx, vy) = sets[0], sets[1]
    assert tx.shape[1] == (9 if stencil else 5)
    P = sr.torch_model(st.initial_weights(seed + model, 1, stencil=stencil)[0] if initial is None else initial, dtype)
    opt = torch.optim.NAdam(P, lr=lr, betas=(0.9, 0.999), eps=1e-7, momentum_decay=4e-3)
    X, Y, VX, VY = [torch.tensor(a.astype(np.float64)).to(dtype) for a in (tx, ty, vx, vy)]
    W, VW = [torch.tensor(np.asarray(a, np.float64)).to(dtype) for a in wsets]
    hist = {k: [] for k in sr.SERIES}
    for e in range(epochs):
        order = torch.from_numpy(st.epoch_permutation(len(tx), seed, model, e))
        tot, tot_abs = 0.0, 0.0
        for s in range(0, len(tx), batch):
            idx = order[s:s + batch]
            opt.zero_grad()
            out = sr.torch_forward(P, X[idx])
            loss = (W[idx, None] * (out - Y[idx]) ** 2).mean()
            loss.backward()
            opt.step()
            tot += float(loss.detach()) * len(idx)
            tot_abs += float((W[idx, None] * (out.detach() - Y[idx]).abs()).mean()) * len(idx)
        hist["loss"].append(tot / len(tx))
        hist["mean_absolute_error"].append(tot_abs / len(tx))
        with torch.no_grad():
            vout = sr.torch_forward(P, VX)
            hist["val_loss"].append(float((VW[:, None] * (vout - VY) ** 2).mean()))
            hist["val_mean_absolute_error"].append(float((VW[:, None] * (vout - VY).abs()).mean()))
    return np.concatenate([p.detach().numpy().ravel() for p in P]).astype(np.float64), hist


def deviations(weights, history, w_ref, hist_ref):
    return sr.deviations(weights, history, w_ref, hist_ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two sample files of the end-to-end tests
N_A, N_B = 600, 60
E2E = dict(epochs=2, batch=64, models=2, seed=5)                          # the end-to-end runs: 2 epochs, batch 64, K = 2
# the continuation of the direction test.  40 epochs = 280 steps: a Nadam step moves a parameter by about lr = 1e-3 at the most, and the
# two runs can only part once the output has travelled the 0.1 .. 0.2 between B's labels and the weighted optimum
CONTINUE = dict(epochs=40, lr=1e-3, heavy=16.0)


def two_files(stencil=False):
    """File A: 600 samples of tests/test_gpu_surrogate_train.py's Kessler-like map over the whole input range; file B: 60 samples from a
    shifted distribution -- cold, thin, dry cells, every input in the lowest fifth of A's range, with a conversion three times as fast.
    B's scaled labels sit near 0, A's spread over [0, 1]: a fit dominated by A pulls the output up and away from B.  Returns
    [(inputs (n, 5, 2), outputs (n, 4))] * 2 in DataGenerator's layout; stencil: slot 1 carries its own values (rain falling in from
    above adds to the precipitation)."""
    lo = np.array([200.0, 0.1, 0.0, 0.0, 0.0])
    hi = np.array([300.0, 1.2, 0.02, 0.004, 0.015])
    out = []
    for n, seed, shifted in ((N_A, 101, False), (N_B, 102, True)):
        rng = np.random.default_rng(seed)
        u = rng.random((n, 5))
        if shifted:
            u *= 0.2
        x = lo + (hi - lo) * u
        above = lo + (hi - lo) * rng.random((n, 5))
        conv = (0.9 if shifted else 0.3) * x[:, 3] * (1.0 + np.tanh((x[:, 0] - 250.0) / 20.0))
        fall = 0.4 * above[:, 3] if stencil else 0.0                   # (row 3 of slot 1: the precipitation above)
        y = np.stack([x[:, 0] + 400.0 * conv, x[:, 2] + 0.2 * conv * x[:, 1], x[:, 3] - conv, x[:, 4] + 0.8 * conv + fall], axis=1)
        out.append((np.stack([x, above], axis=2).astype(np.float32), y.astype(np.float32)))
    return out


def two_file_arrays(stencil=False):
    """(features (660, 5 | 9), outputs (660, 4), file index (660,)) of two_files, as read_samples concatenates them."""
    from miniweatherml_amd import surrogate_train as st
    files = two_files(stencil)
    feats = [np.concatenate([i3[:, :, 0], i3[:, st.ABOVE_ROWS, 1]], axis=1) if stencil else np.ascontiguousarray(i3[:, :, 0]) for i3, _ in files]
    return np.concatenate(feats), np.concatenate([o for _, o in files]), np.repeat(np.arange(2), [N_A, N_B])


def file_test_loss(w, sets, gsets, g):
    """The unweighted loss of the weights w on file g's samples of the test set, by the fp64 forward."""
    sx, sy = sets[2]
    pick = gsets[2] == g
    out = sr.forward64(w, sx[pick])[1]
    return float(np.mean((out - sy[pick].astype(np.float64)) ** 2))


def direction_replay(dtype=None):
    """The direction test on the CPU: the fp64 replay of the (1, 1) run's model 0, continued (its weights as the start, Nadam from zero,
    model 0's shuffles) with file weights (1, 1) and (1, heavy).  Returns the two unweighted test losses on file B."""
    import torch
    dtype = dtype or torch.float64
    x, y, gi = two_file_arrays()
    seed = E2E["seed"]
    sets = sr.host_sets(x, y, seed)
    from miniweatherml_amd import surrogate_train as st
    n_train, n_val, _ = st.split_sizes(len(x))
    gsets = split_column(gi, seed, n_train, n_val)
    ones = (np.ones(n_train), np.ones(n_val))
    w_a, _ = replay(dtype, sets, ones, seed, E2E["batch"], E2E["epochs"])
    res = []
    for heavy in (1.0, CONTINUE["heavy"]):
        fw = np.array([1.0, heavy])
        w_c, _ = replay(dtype, sets, (fw[gsets[0]], fw[gsets[1]]), seed, E2E["batch"], CONTINUE["epochs"], CONTINUE["lr"], initial=w_a)
        res.append(file_test_loss(w_c, sets, gsets, 1))
    return tuple(res)
