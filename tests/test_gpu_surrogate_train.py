"""Surrogate training on the MI355X (miniweatherml_amd/surrogate_train.py, csrc/mw_train.hip): the batch gradient against torch fp64
autograd, a two-epoch trajectory against torch fp64 NAdam replaying the product's batch order, determinism, independence of the models
trained together, and generate -> train -> infer end to end on the project's own Kessler data."""
import json
import os

import numpy as np
import pytest

from surrogate_ref import (GRAD_BATCHES, check_rho, check_test_metrics, deviations, device_batch_grad, gradient_case, host_sets, replay,
                           signs_ok, torch_forward, torch_model)
from test_surrogate_train_cpu import write_sample_file
from util import push_fields

pytestmark = pytest.mark.gpu


def kessler_like(n, seed):
    """Synthetic samples in DataGenerator's layout with Kessler-like ranges and a smooth nonlinear input -> output map."""
    rng = np.random.default_rng(seed)
    lo = np.array([200.0, 0.1, 0.0, 0.0, 0.0])
    hi = np.array([300.0, 1.2, 0.02, 0.004, 0.015])
    x = lo + (hi - lo) * rng.random((n, 5))
    conv = 0.3 * x[:, 3] * (1.0 + np.tanh((x[:, 0] - 250.0) / 20.0))
    y = np.stack([x[:, 0] + 400.0 * conv, x[:, 2] + 0.2 * conv * x[:, 1], x[:, 3] - conv, x[:, 4] + 0.8 * conv], axis=1)
    ins = np.repeat(x[:, :, None], 2, axis=2)
    return ins.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("batch", GRAD_BATCHES)
def test_batch_gradient_matches_torch_autograd(mw, batch):
    """Batch sizes where the masking, the wave split and the chunk loop change shape: one sample, below one wave, around 64 and 256, and
    MW_SURROGATE_MAX_BATCH.  fp32 summation in the worst order stays at or below 2.4e-6 of max|g| for every one of them (CPU), torch
    fp32's loss at or below 2.3e-7: the two bounds hold for any order.  rho is the per-entry statement (tests/surrogate_ref.py)."""
    import torch
    w, x, y = gradient_case(5, batch)
    g, loss = device_batch_grad(5, w, x, y, v2=False)
    P = torch_model(w)
    xt = torch.tensor(x.T.astype(np.float64))
    assert signs_ok(5, w, x)
    ref = torch.nn.functional.mse_loss(torch_forward(P, xt), torch.tensor(y.T.astype(np.float64)))
    ref.backward()
    g_ref = np.concatenate([p.grad.numpy().ravel() for p in P])
    check_rho(5, w, x, y, g, "single cell, batch %d" % batch)
    assert np.max(np.abs(g - g_ref)) <= 1e-5 * np.max(np.abs(g_ref)), np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref))
    assert abs(loss - float(ref.detach())) <= 1e-6 * float(ref.detach())


@pytest.fixture(scope="module")
def file20k(tmp_path_factory):
    ins, outs = kessler_like(20000, 1)
    return write_sample_file(tmp_path_factory.mktemp("s20k") / "s.nc", [(ins[:7000], outs[:7000]), (ins[7000:], outs[7000:])]), ins, outs


# max|dw| / max|w|, then loss, val_loss, mean_absolute_error, val_mean_absolute_error (largest relative deviation over the epochs).
# Measured on the MI355X: 2.99e-7, 3.49e-8, 8.51e-9, 2.78e-8, 5.15e-9; bounds = 3 x measured, rounded up to one digit.  torch's fp32
# replay on the CPU deviates from the fp64 one by 2.5e-7, 8.1e-9, 1.0e-7, 7.2e-9, 2.7e-8 (tests/surrogate_ref.py: replay).
TRAJECTORY_BOUNDS = (9e-7, 2e-7, 3e-8)
MAE_BOUNDS = (9e-8, 2e-8)


def test_two_epoch_trajectory_matches_torch_nadam(mw, file20k):
    """2 epochs on 20,000 samples at batch 1024 (12,800 training samples: 13 steps per epoch, the last one partial) from the product's
    seeded initial weights in the product's batch order, against torch fp64 (Linear -> leaky_relu(0.1) -> Linear, mse_loss, NAdam(eps=1e-7,
    momentum_decay=4e-3)).  First bounds (>= 3x the first run: max|dw| = 5.9e-6 of max|w|, loss 5.9e-7, val_loss 9.3e-7 relative): 2e-5,
    2e-6, 3e-6.  Those figures were 23 times torch fp32's own deviation: the bias correction was built from beta2 = 0.999 while the kernel
    runs fp32(0.999) (surrogate_train.kernel_nadam_table).  With that mended the run stays at fp32's level; both sets of bounds are
    asserted, TRAJECTORY_BOUNDS being the tighter."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    path, ins, outs = file20k
    seed = 5
    r = st.train_surrogate([path], epochs=2, batch_size=1024, seed=seed)
    (tx, ty), (vx, vy), _ = host_sets(ins[:, :, 0], outs, seed)
    assert (r["n_train"], r["n_val"], r["n_test"]) == (12800, 3200, 4000) and len(tx) == 12800
    w_ref, h_ref = replay(torch.float64, [(tx, ty), (vx, vy)], seed, 1024, 2, 1e-3, stencil=False)
    w = r["weights"][0].astype(np.float64)
    dw, dl, dm, dv, dvm = deviations(w, r["history"][0], w_ref, h_ref)
    print("trajectory: max|dw|/max|w| %.2e, loss %.2e, val_loss %.2e, mean_absolute_error %.2e, val_mean_absolute_error %.2e" % (dw, dl, dv, dm, dvm))
    assert dw <= 2e-5 and dl <= 2e-6 and dv <= 3e-6
    assert dw <= TRAJECTORY_BOUNDS[0] and dl <= TRAJECTORY_BOUNDS[1] and dv <= TRAJECTORY_BOUNDS[2]
    assert dm <= MAE_BOUNDS[0] and dvm <= MAE_BOUNDS[1]
    assert np.max(np.abs(w - st.initial_weights(seed, 1)[0])) > 5e-3           # it moved


def test_training_is_deterministic(mw, file20k):
    from miniweatherml_amd import surrogate_train as st
    a = st.train_surrogate([file20k[0]], epochs=2, batch_size=512, seed=3, models=2)
    b = st.train_surrogate([file20k[0]], epochs=2, batch_size=512, seed=3, models=2)
    assert np.array_equal(a["weights"].view(np.uint32), b["weights"].view(np.uint32))
    assert a["history"] == b["history"] and a["test_metrics"] == b["test_metrics"]


def test_models_are_independent_of_each_other(mw, file20k):
    """Model m of a K = 4 run is bitwise the K = 1 run of seed + m on the same split."""
    from miniweatherml_amd import surrogate_train as st
    r4 = st.train_surrogate([file20k[0]], epochs=2, batch_size=1000, seed=10, models=4)
    assert r4["seeds"] == [10, 11, 12, 13] and r4["split_seed"] == 10
    for m in (0, 2):
        r1 = st.train_surrogate([file20k[0]], epochs=2, batch_size=1000, seed=10 + m, models=1, split_seed=10)
        assert (r1["n_train"], r1["n_val"], r1["n_test"], r1["split_seed"]) == (r4["n_train"], r4["n_val"], r4["n_test"], 10)
        assert np.array_equal(r1["weights"][0].view(np.uint32), r4["weights"][m].view(np.uint32))
        assert r1["history"][0] == r4["history"][m]
    final = [h["val_loss"][-1] for h in r4["history"]]
    assert r4["best_model"] == int(np.argmin(final))
    assert len(set(final)) == 4


def rainy_state(oracle, nx, ny, nz):
    """The recipe of test_gpu_kessler_mlp.rainy_state (heavy = False): an oracle supercell state pushed into cloud and rain."""
    dyc, f = oracle.supercell_setup(nx, ny, nz, 1, 500.0 * nx, 500.0 * ny, 20000.)
    rng = np.random.default_rng(11)
    shp = f.rho_d.shape
    f.tracers[1][...] = rng.uniform(0, 3e-3, shp) * (rng.uniform(size=shp) > 0.4) * f.rho_d
    f.tracers[2][...] = rng.uniform(0, 5e-4, shp) * (rng.uniform(size=shp) > 0.5) * f.rho_d
    f.tracers[0][...] *= rng.uniform(0.6, 1.3, shp)
    return f


def test_generate_train_infer_end_to_end(mw, oracle, tmp_path):
    """DataGenerator's file of every cell of a rainy supercell state after the GPU Kessler (131,072 samples), 10 epochs at batch 256, then
    the written files through load_surrogate_weights into mlp_forward, against the oracle's forward with the same weights and scaling.
    Measured on the MI355X (first run): final val_loss 7.3e-4 = 1/70 of the variance baseline 5.1e-2; asserted: 1/20 (3.5x margin)."""
    from miniweatherml_amd import modules, surrogate_train as st
    from miniweatherml_amd.coupler import Coupler
    from util import gpu_fields
    nx, ny, nz = 64, 64, 32
    f = rainy_state(oracle, nx, ny, nz)
    coupler, dycore, micro = modules.make_supercell(nx, ny, nz, 1, 500.0 * nx, 500.0 * ny, 20000.)
    push_fields(coupler, f)
    dt = dycore.compute_time_step(coupler)
    inp = Coupler("cuda:0")
    coupler.clone_into(inp)
    micro.time_step(coupler, dt)
    gen = modules.DataGenerator()
    gen.desired_samples_per_time_step = 1e12                           # every cell
    gen.init(coupler, str(tmp_path))
    n = gen.generate_samples_stencil(inp, coupler, dt, 0.0, seed=1)
    assert n == nx * ny * nz
    out_dir = str(tmp_path / "trained")
    r = st.train_surrogate([gen.fname], out_dir=out_dir, epochs=10, batch_size=256, seed=0)
    assert r["time_step_size"] == dt and r["dx"] == inp.get_dx()
    (tx, ty), _, _ = host_sets(*st.read_samples([gen.fname])[:2], 0)
    baseline = float(np.mean(np.var(ty.astype(np.float64), axis=0)))
    ratio = r["history"][0]["val_loss"][-1] / baseline
    print("val_loss %.3e, variance baseline %.3e, ratio 1/%.0f" % (r["history"][0]["val_loss"][-1], baseline, 1.0 / ratio))
    assert ratio <= 1.0 / 20
    paths = [os.path.join(out_dir, p) for p in ("weights.txt", "input_scaling.txt", "output_scaling.txt")]
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights(weights_txt=paths[0], in_scaling_txt=paths[1], out_scaling_txt=paths[2])
    assert np.array_equal(np.concatenate([W1.ravel(), b1, W2.ravel(), b2]), r["weights"][0])
    dm = inp.get_data_manager_readwrite()
    outs = modules.mlp_forward(dm.get("temp"), dm.get("density_dry"), dm.get("water_vapor"), dm.get("cloud_liquid"), dm.get("precip_liquid"),
                               W1, b1, W2, b2, si, so)
    g = gpu_fields(inp)
    ref = oracle.mlp_forward(g["temp"], g["density_dry"], g["tracer0"], g["tracer1"], g["tracer2"], W1, b1, W2, b2, si, so)
    for k, (o, rr) in enumerate(zip(outs, ref)):
        assert np.max(np.abs(o.cpu().numpy() - rr)) <= 1e-5 * (so[k, 1] - so[k, 0]), k
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "surrogate_notebook_metrics.json")))
    tm = r["test_metrics"]
    ref = check_test_metrics(r, host_sets(*st.read_samples([gen.fname])[:2], 0)[2], "end to end")
    for key in ("max_relative_error", "mean_relative_error"):
        print("%-20s here %s | notebook %s" % (key, np.array2string(np.array(tm[key]), precision=5), golden[key.replace("error", "test_errors")]))
    assert np.all(ref["max_relative_error"] > 0) and np.all(ref["mean_relative_error"] > 0)
    assert json.load(open(os.path.join(out_dir, "history.json")))["best_model"] == 0
