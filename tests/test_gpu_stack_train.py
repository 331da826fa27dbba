"""Native training of dense surrogate stacks on the MI355X (csrc/mw_train_stack.hip): the batch gradient against
an fp64 statement of the network, a short trajectory against an fp64 torch Nadam replay, determinism and the independence of the models,
and train_surrogate(stack=...) end to end.  The references are the plain numpy / torch functions of this file."""
import ctypes

import numpy as np
import pytest

import surrogate_ref as sr
from test_gpu_surrogate_train import kessler_like
from test_surrogate_train_cpu import write_sample_file

pytestmark = pytest.mark.gpu

SLOPES = (0.1, 0.0, 1.0, 0.25)
SWEEP = (1, 15, 16, 17, 63, 64, 65, 257)                                  # below / at / above a 16-sample tile, the four waves, many tiles
GRAD_CASES = [(n_in, h, b) for n_in, h in ((5, [5]), (5, [17]), (9, [10])) for b in SWEEP] + \
             [(5, [1], 65), (5, [4], 257), (5, [15], 65), (5, [16], 257), (5, [33], 65), (5, [64], 257), (9, [17, 3, 64], 257),
              (5, [64, 64, 64, 64], 257), (9, [64, 64, 64, 64], 65), (5, [17, 3], 8192)]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stack_case(n_in, hidden, batch):
    """surrogate_ref.gradient_case for a stack: weights N(0, 0.6 sqrt(5 / fan_in)) (pre-activations of order one at every width), the
    hidden biases shifted by -0.5, x and y uniform in [0, 1), sample weights 2^U(-4, 4) with every seventh exactly 0."""
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng([batch, n_in] + hidden)
    widths = [n_in] + hidden + [4]
    slopes = np.array([SLOPES[(l + batch) % 4] for l in range(len(hidden))], np.float32)
    parts = []
    for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        parts += [rng.standard_normal(a * b) * 0.6 * np.sqrt(5.0 / max(5, a)), np.zeros(b) - (0.5 if l < len(hidden) else 0.0)]
    w = np.concatenate(parts).astype(np.float32)
    assert w.size == st.stack_n_params(widths)
    x, y = rng.random((n_in, batch), dtype=np.float32), rng.random((4, batch), dtype=np.float32)
    wt = (2.0 ** rng.uniform(-4, 4, batch)).astype(np.float32)
    wt[3::7] = 0.0
    return widths, slopes, w, x, y, wt


def grad64(widths, slopes, w, x, y, wt):
    """fp64: (gradient of sum_i wt_i mean_o((out - t)^2) / B, T = 0.5 / B sum_l |a_{l-1}|^T |delta_l| per entry, loss, pre-activations)."""
    from miniweatherml_amd import surrogate_train as st
    L = st.split_stack_weights(np.asarray(w, np.float64), widths)
    a, pre = [np.asarray(x, np.float64).T], []
    for l, (W, b) in enumerate(L):
        z = a[-1] @ W + b
        pre.append(z)
        a.append(np.where(z > 0, z, float(slopes[l]) * z) if l < len(L) - 1 else z)
    B = a[0].shape[0]
    r = a[-1] - np.asarray(y, np.float64).T
    d = r * np.asarray(wt, np.float64)[:, None]
    g, T = [], []
    for l in range(len(L) - 1, -1, -1):
        g = [a[l].T @ d, d.sum(0)] + g
        T = [np.abs(a[l]).T @ np.abs(d), np.abs(d).sum(0)] + T
        if l:
            d = (d @ L[l][0].T) * np.where(pre[l - 1] > 0, 1.0, float(slopes[l - 1]))
    flat = lambda v: np.concatenate([p.ravel() for p in v]) * 0.5 / B        # noqa: E731
    return flat(g), flat(T), float((np.asarray(wt, np.float64) * (r * r).sum(1)).sum() / (4 * B)), pre[:-1]


def torch_stack(P, slopes, x):
    import torch
    for l in range(0, len(P) - 2, 2):
        x = torch.nn.functional.leaky_relu(x @ P[l] + P[l + 1], float(slopes[l // 2]))
    return x @ P[-2] + P[-1]


def torch_params(w, widths, dtype):
    import torch
    from miniweatherml_amd import surrogate_train as st
    return [torch.tensor(np.array(p, np.float64)).to(dtype).requires_grad_() for Wb in st.split_stack_weights(w, widths) for p in Wb]


def grad32_torch(widths, slopes, w, x, y, wt):
    import torch
    P = torch_params(w, widths, torch.float32)
    out = torch_stack(P, slopes, torch.tensor(x.T.copy()))
    loss = (torch.tensor(wt) * ((out - torch.tensor(y.T.copy())) ** 2).mean(1)).sum() / x.shape[1]
    loss.backward()
    return np.concatenate([p.grad.numpy().ravel() for p in P]).astype(np.float64)


def device_grad(widths, slopes, w, x, y, wt):
    import torch
    from miniweatherml_amd import capi
    L, B, hidden = capi.lib(), x.shape[1], (ctypes.c_int * (len(widths) - 2))(*widths[1:-1])
    nb = L.mw_stack_train_workspace_bytes(widths[0], len(hidden), hidden, 1, B)
    assert nb > 0
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (w, x, y)]
    dwt = None if wt is None else torch.from_numpy(wt).cuda()
    grad = torch.full((w.size,), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    capi.check(L.mw_stack_batch_grad(widths[0], len(hidden), hidden, slopes.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ptr(dev[0]), ptr(dev[1]),
                                     ptr(dev[2]), None if wt is None else ptr(dwt), B, ptr(grad), ptr(loss), ptr(ws), None))
    torch.cuda.synchronize()
    return grad.cpu().numpy().astype(np.float64), float(loss.cpu()[0])


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("n_in,hidden,batch", GRAD_CASES)
def test_stack_batch_gradient_matches_fp64(mw, n_in, hidden, batch, weighted):
    """mw_stack_batch_grad against grad64 by the trainer's own criterion (surrogate_ref.check_rho): rho(kernel) <= 4 rho(torch fp32 autograd
    on the CPU), max|g - g_ref| <= 1e-5 max|g_ref|, loss to 1e-6.  grad has exactly nparams entries: a padded unit has none."""
    widths, slopes, w, x, y, wt = stack_case(n_in, hidden, batch)
    if not weighted:
        wt = np.ones(batch, np.float32)
    g_ref, T, loss_ref, pre = grad64(widths, slopes, w, x, y, wt)
    assert all((p > 0).any() and (p < 0).any() for p in pre), "both branches of every hidden layer"
    g, loss = device_grad(widths, slopes, w, x, y, wt if weighted else None)
    assert g.shape == g_ref.shape and np.isfinite(g).all()
    live = T > 0
    assert np.all(g[~live] == 0)                                          # (e.g. every sample of weight zero)
    got, cpu = sr.rho(g[live], g_ref[live], T[live]), sr.rho(grad32_torch(widths, slopes, w, x, y, wt)[live], g_ref[live], T[live])
    err = np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref))
    print("%r B %d weighted %d: rho(kernel) %.1f, rho(torch fp32) %.1f, max|dg|/max|g| %.2e, loss rel %.2e"
          % (widths, batch, weighted, got, cpu, err, abs(loss - loss_ref) / loss_ref))
    assert got <= 4.0 * cpu, (got, cpu)
    assert err <= 1e-5
    assert abs(loss - loss_ref) <= 1e-6 * loss_ref


# ---------------------------------------------------------------------------------------------------------------------------------
def sample_files(tmp_path, n, stencil):
    ins, outs = kessler_like(n, 11)
    if stencil:
        ins = ins.copy()
        ins[:, :, 1] *= np.float32(0.97)                                   # a level above that differs from the cell
    path = tmp_path / "samples.nc"
    write_sample_file(path, [(ins, outs)])
    return [str(path)]


def run(files, hidden, stencil=False, **kw):
    from miniweatherml_amd import surrogate_train as st
    return st.train_surrogate(files, None, epochs=kw.pop("epochs", 2), batch_size=300, seed=5, stack=hidden, slopes=kw.pop("slopes", 0.1), stencil=stencil, **kw)


def test_stack_training_is_deterministic_and_models_are_independent(mw, tmp_path):
    """The same call twice: the same bits.  K = 3: every model has the bits and the history of its seed trained alone."""
    files = sample_files(tmp_path, 2000, False)
    three, again = run(files, [33, 5], models=3), run(files, [33, 5], models=3)
    assert np.array_equal(three["weights"].view(np.uint32), again["weights"].view(np.uint32)) and three["history"] == again["history"]
    for k in range(3):
        from miniweatherml_amd import surrogate_train as st
        alone = st.train_surrogate(files, None, epochs=2, batch_size=300, seed=5 + k, split_seed=5, stack=[33, 5])
        assert np.array_equal(alone["weights"][0].view(np.uint32), three["weights"][k].view(np.uint32)), k
        assert alone["history"][0] == three["history"][k], k


def test_train_surrogate_stack_end_to_end(mw, tmp_path, capsys, monkeypatch):
    """train_surrogate(stack=[16, 16]) -> files -> load_surrogate_stack: the best model's bits; mlp_stack_forward on the test samples agrees
    with Trainer.predict_test to 1e-5 of each output's range; the loss falls; the CLI writes the header and the form marker."""
    import torch
    from miniweatherml_amd import mlp, surrogate_train as st
    files = sample_files(tmp_path, 3000, False)
    out = tmp_path / "model"
    r = st.train_surrogate(files, str(out), epochs=3, batch_size=256, seed=2, stack=[16, 16])
    stack = mlp.load_surrogate_stack(*r["files_written"])
    flat = np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in stack.layers])
    assert np.array_equal(flat.view(np.uint32), r["weights"][r["best_model"]].view(np.uint32))
    assert mlp.stack_widths(stack) == [5, 16, 16, 4] and r["stack"] == [16, 16]
    h = r["history"][r["best_model"]]["loss"]
    assert h[-1] < h[0]
    # the test split through the trainer's own predictor and through the model loop's kernel
    inputs, outputs, _ = st.read_samples(files)
    n_split = st.check_arguments(inputs.shape[0], 3, 256, 0.2, 0.2, 1)
    tr = st.Trainer(torch.from_numpy(inputs).cuda(), torch.from_numpy(outputs).cuda(), r["input_scaling"], r["output_scaling"], n_split, seed=2,
                    batch_size=256, epochs=1, stack=[16, 16])
    pred = tr.predict_test(r["weights"][r["best_model"]]).cpu().numpy().astype(np.float64)
    lo, rng = r["output_scaling"][:, 0:1], (r["output_scaling"][:, 1] - r["output_scaling"][:, 0])[:, None]
    want = pred * rng + lo
    want[1:] = np.maximum(want[1:], 0.0)                                  # the model loop clips the three water fields
    raw = inputs[st.preshuffle_permutation(inputs.shape[0], 2)[n_split[0] + n_split[1]:]].astype(np.float64)
    fields = [torch.from_numpy(np.ascontiguousarray(raw[:, f])).cuda() for f in range(5)]
    got = np.stack([o.cpu().numpy() for o in mlp.mlp_stack_forward(stack, 1, *fields)])
    err = np.max(np.abs(got - want) / rng, axis=1)
    print("mlp_stack_forward against predict_test, per output, in units of the range:", err)
    assert np.all(err <= 1e-5)
    # the command line: stencil, tendency
    out2 = tmp_path / "cli"
    assert st.main(files + ["--out", str(out2), "--epochs", "1", "--stack", "16,16", "--stencil", "--tendency"]) == 0
    assert "inference_ponni" in capsys.readouterr().out
    assert mlp.stack_header(str(out2 / "weights.txt")) == ([9, 16, 16, 4], [pytest.approx(0.1)] * 2)
    assert open(out2 / "output_scaling.txt").readline().strip() == st.FORM_MARKER
    # init=DIR with the same shape and slopes: every model starts at DIR's bits, keeps DIR's scaling tables and moves on
    r2 = st.train_surrogate(files, None, epochs=1, batch_size=256, seed=9, stack=[16, 16], init=str(out))
    assert np.array_equal(r2["initial_weights"][0].view(np.uint32), flat.view(np.uint32)) and np.array_equal(r2["input_scaling"], stack.scl_in)
    assert np.max(np.abs(r2["weights"][0] - flat)) > 1e-4
    # the driver's path through the `# stack:` header: inference_ponni on the trained directory
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver
    extra = "".join('%s: "%s"\n' % kv for kv in zip(("keras_weights_txt", "nn_input_scaling", "nn_output_scaling"), r["files_written"]))
    path, _ = write_yaml(tmp_path, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    driver.run("inference_ponni", path, max_steps=2, quiet=False)
    diffs = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Relative diff")]
    print("\n".join(diffs))
    assert len(diffs) == 8 and all(np.isfinite(float(ln.split()[-1])) for ln in diffs)


# ---------------------------------------------------------------------------------------------------------------------------------
# Trajectory against the torch fp64 Nadam replay: 2,000 kessler_like samples, batch 300 (1280 training samples: four full batches of more
# than one 256-sample pass and a partial one of 80), 2 epochs.  MEASURED on the MI355X, the largest relative deviation of each series
# over the epochs (loss, mean_absolute_error, val_loss, val_mean_absolute_error); the bounds are 3 x measured, rounded up to one digit:
#   shape                     max|dw|/max|w|  loss      mae       val_loss  val_mae
#   5-10            kernel      2.07e-07      2.03e-07  4.20e-08  8.15e-08  5.06e-08
#                   fp32 replay 2.68e-07      1.32e-07  7.39e-08  1.81e-07  6.88e-08
#   9-17-3 weighted kernel      9.03e-08      1.55e-07  1.71e-07  2.89e-08  1.05e-08
#                   fp32 replay 1.43e-07      1.42e-07  6.26e-08  1.21e-07  1.57e-08
#   5-64x4 tendency kernel      2.09e-07      2.69e-07  1.77e-07  2.43e-08  1.73e-08
#                   fp32 replay 2.82e-07      1.57e-07  8.31e-08  1.73e-07  1.10e-07
# (the weights are held to 4 x the fp32 replay's own deviation, computed in the test; they moved 8.7e-3 to 1.3e-2 from their start)
TRAJ_CASES = [((5, [10]), dict(), (7e-7, 2e-7, 3e-7, 2e-7)),
              ((9, [17, 3]), dict(weighted=True), (5e-7, 6e-7, 9e-8, 4e-8)),
              ((5, [64, 64, 64, 64]), dict(form="tendency"), (9e-7, 6e-7, 8e-8, 6e-8))]


def replay(dtype, widths, slopes, sets, wsets, seed, batch, epochs):
    """torch NAdam(eps=1e-7, momentum_decay=4e-3) on mse (Keras' sample_weight reduction) from the trainer's initial weights in
    st.epoch_permutation's order; returns (weights fp64, the four series)."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    T = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)          # noqa: E731
    P = torch_params(st.stack_initial_weights(seed, 1, widths)[0], widths, dtype)
    opt = torch.optim.NAdam(P, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, momentum_decay=4e-3)
    (X, Y, W), (VX, VY, VW) = [(T(x.T), T(y.T), T(w)) for (x, y), w in zip(sets, wsets)]
    hist = {k: [] for k in sr.SERIES}
    for e in range(epochs):
        order = torch.from_numpy(st.epoch_permutation(len(X), seed, 0, e))
        tot = tot_abs = 0.0
        for s in range(0, len(X), batch):
            idx = order[s:s + batch]
            opt.zero_grad()
            out = torch_stack(P, slopes, X[idx])
            loss = (W[idx] * ((out - Y[idx]) ** 2).mean(1)).sum() / len(idx)
            loss.backward()
            opt.step()
            tot += float(loss.detach()) * len(idx)
            tot_abs += float((W[idx] * (out.detach() - Y[idx]).abs().mean(1)).sum())
        with torch.no_grad():
            vout = torch_stack(P, slopes, VX)
            hist["loss"].append(tot / len(X))
            hist["mean_absolute_error"].append(tot_abs / len(X))
            hist["val_loss"].append(float((VW * ((vout - VY) ** 2).mean(1)).sum() / len(VX)))
            hist["val_mean_absolute_error"].append(float((VW * (vout - VY).abs().mean(1)).sum() / len(VX)))
    return np.concatenate([p.detach().numpy().ravel() for p in P]).astype(np.float64), hist


@pytest.mark.parametrize("shape,kw,bounds", TRAJ_CASES, ids=["5-10", "9-17-3-weighted", "5-64x4-tendency"])
def test_stack_trajectory_follows_the_fp64_replay(mw, tmp_path, shape, kw, bounds):
    import torch
    from miniweatherml_amd import surrogate_train as st
    (n_in, hidden), seed, batch, epochs = shape, 3, 300, 2
    files = sample_files(tmp_path, 2000, n_in == 9)
    wt = (2.0 ** np.random.default_rng(1).uniform(-4, 4, 2000)).astype(np.float32) if kw.get("weighted") else None
    form = kw.get("form", "state")
    r = st.train_surrogate(files, None, epochs=epochs, batch_size=batch, seed=seed, stack=hidden, stencil=n_in == 9, form=form, sample_weights=wt)
    inputs, outputs, _ = st.read_samples(files, stencil=n_in == 9)
    n_split = (r["n_train"], r["n_val"], r["n_test"])
    tr = st.Trainer(torch.from_numpy(inputs).cuda(), torch.from_numpy(outputs).cuda(), r["input_scaling"], r["output_scaling"], n_split, seed=seed,
                    batch_size=batch, epochs=1, stack=hidden, form=form, sample_weights=wt)
    sets = [tuple(t.cpu().numpy() for t in tr.sets[k]) for k in ("train", "val")]
    wsets = [np.ones(s[0].shape[1], np.float32) if wt is None else tr.wsets[k].cpu().numpy() for s, k in zip(sets, ("train", "val"))]
    widths, slopes = st.stack_shape(hidden, 0.1, stencil=n_in == 9)
    w64, h64 = replay(torch.float64, widths, slopes, sets, wsets, seed, batch, epochs)
    w32, h32 = replay(torch.float32, widths, slopes, sets, wsets, seed, batch, epochs)
    dev, yard = sr.deviations(r["weights"][0], r["history"][0], w64, h64), sr.deviations(w32, h32, w64, h64)
    moved = float(np.max(np.abs(r["weights"][0] - st.stack_initial_weights(seed, 1, widths)[0])))      # the kernel's own weights
    print("%r kernel      %s\n%s fp32 replay %s   moved %.2e" % (widths, " ".join("%.2e" % v for v in dev), " " * len(repr(widths)),
                                                                  " ".join("%.2e" % v for v in yard), moved))
    assert moved > 5e-3
    assert dev[0] <= 4.0 * yard[0], (dev[0], yard[0])
    for v, b in zip(dev[1:], bounds):
        assert v <= b, (dev, bounds)
