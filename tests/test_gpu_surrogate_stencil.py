"""The two-cell stencil surrogate (9 -> 10 -> 4) on the MI355X: the inference kernels (csrc/mw_mlp.hip: k_mlp_stencil, k_mlp_stencil_strict)
against a numpy restatement, the trainer's stencil instantiation (csrc/mw_train.hip) against torch fp64, and generate -> train -> infer
with the model in the loop.  The oracle has no stencil model: the yardsticks are written here."""
import ctypes
import json
import os

import numpy as np
import pytest

from surrogate_ref import (GRAD_BATCHES, check_rho, check_test_metrics, deviations, device_batch_grad, gradient_case, host_sets, replay,
                           signs_ok, torch_forward, torch_model)
from test_surrogate_train_cpu import write_sample_file
from util import push_fields

pytestmark = pytest.mark.gpu

FIELDS = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")


def mlp_tol(scl_out, n):
    return 1e-5 * (scl_out[n, 1] - scl_out[n, 0])                   # tests/test_gpu_kessler_mlp.py: 1e-5 on the fp32 network output


def np_stencil_forward(fields, nz, W1, b1, W2, b2, si, so):
    """ponni's Matvec, Bias, Relu(0.1), Matvec, Bias in fp32, index order, one rounding per operation, on the nine scaled features
    (fp64 quotient rounded to fp32); un-scaling in fp64 and the >= 0 clip of the three densities.  Returns four flat fp64 arrays."""
    from miniweatherml_amd import modules
    X = modules.stencil_features(fields, nz)
    x = ((X - si[:, 0:1]) / (si[:, 1:2] - si[:, 0:1])).astype(np.float32)
    W1, b1, W2, b2 = [np.asarray(a, np.float32) for a in (W1, b1, W2, b2)]
    h = []
    for o in range(10):
        acc = np.zeros(x.shape[1], np.float32)
        for i in range(9):
            acc = acc + x[i] * W1[i, o]
        acc = acc + b1[o]
        h.append(np.where(acc > 0, acc, np.float32(0.1) * acc))
    outs = []
    for o in range(4):
        acc = np.zeros(x.shape[1], np.float32)
        for i in range(10):
            acc = acc + h[i] * W2[i, o]
        acc = acc + b2[o]
        assert acc.dtype == np.float32
        y = acc.astype(np.float64) * (so[o, 1] - so[o, 0]) + so[o, 0]
        outs.append(y if o == 0 else np.maximum(0.0, y))
    return outs


def random_stencil_net(seed, si5=None):
    """A network of the shipped one's magnitude with all nine rows of W1 alive, and a nine-row scaling table."""
    from miniweatherml_amd import modules
    W1s, b1, W2, b2, si, so = modules.load_surrogate_weights()
    rng = np.random.default_rng(seed)
    W1 = np.concatenate([W1s, rng.permutation(W1s[[0, 2, 3, 4]].ravel()).reshape(4, 10)]).astype(np.float32)
    si9 = np.concatenate([si, si[[0, 2, 3, 4]] * np.array([[0.97, 1.02]])])          # the level-above features scale differently
    return np.ascontiguousarray(W1), b1, W2, b2, np.ascontiguousarray(si9), so


def rainy_state(oracle, nx, ny, nz):
    """An oracle supercell state pushed into cloud and rain (the recipe of tests/test_gpu_surrogate_train.py)."""
    dyc, f = oracle.supercell_setup(nx, ny, nz, 1, 500.0 * nx, 500.0 * ny, 20000.)
    rng = np.random.default_rng(11)
    shp = f.rho_d.shape
    f.tracers[1][...] = rng.uniform(0, 3e-3, shp) * (rng.uniform(size=shp) > 0.4) * f.rho_d
    f.tracers[2][...] = rng.uniform(0, 5e-4, shp) * (rng.uniform(size=shp) > 0.5) * f.rho_d
    f.tracers[0][...] *= rng.uniform(0.6, 1.3, shp)
    return f


def run_both(fields, nz, net):
    """(strict outputs, production outputs) as flat numpy arrays."""
    import torch
    from miniweatherml_amd import modules
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in fields]
    strict = [o.cpu().numpy().ravel() for o in modules.mlp_stencil_forward(nz, *t, *net, strict=1)]
    fast = [o.cpu().numpy().ravel() for o in modules.mlp_stencil_forward(nz, *t, *net)]
    return strict, fast


def check_against_restatement(fields, nz, net, what):
    ref = np_stencil_forward(fields, nz, *net)
    strict, fast = run_both(fields, nz, net)
    so = net[5]
    for n in range(4):
        assert np.array_equal(strict[n], ref[n]), (what, n, np.max(np.abs(strict[n] - ref[n])))
        err = np.max(np.abs(fast[n] - ref[n]))
        assert err <= mlp_tol(so, n), (what, n, err / mlp_tol(so, n))
    for n in (1, 2, 3):
        assert strict[n].min() >= 0.0 and fast[n].min() >= 0.0


def test_stencil_forward_on_supercell_state_and_beyond_the_ranges(mw, oracle):
    """Strict: bit-identical to the restatement.  Production (MFMA, top-down sweep): within 1e-5 of the output range."""
    net = random_stencil_net(1)
    f = rainy_state(oracle, 20, 16, 24)
    check_against_restatement([f.temp, f.rho_d, f.tracers[0], f.tracers[1], f.tracers[2]], 24, net, "supercell")
    si = net[4]
    rng = np.random.default_rng(3)
    nz, ncol = 23, 2175
    wide = [rng.uniform(si[i, 0] - 0.2 * (si[i, 1] - si[i, 0]), si[i, 1] + 0.2 * (si[i, 1] - si[i, 0]), (nz, ncol)) for i in range(5)]
    check_against_restatement(wide, nz, net, "beyond the ranges")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 11, 1), (2, 1, 15, 1), (2, 5, 7, 2), (22, 1, 17, 1), (22, 3, 11, 2), (37, 25, 40, 1),
                                   (9, 1, 1, 1), (13, 9, 9, 2)])
def test_stencil_forward_ragged_shapes(mw, shape):
    """nz = 1, 2 and values that no z chunk divides; ncol = ny nx nens that are not multiples of 16 or 32; nens = 2."""
    from miniweatherml_amd import capi
    nz, ny, nx, nens = shape
    ncol = ny * nx * nens
    zc = capi.lib().mw_mlp_stencil_chunk(nz, ncol)
    assert 1 <= zc <= nz
    if nz >= 22:
        assert zc < nz and nz % zc != 0, (nz, zc)                    # several chunks, the last one shorter
    net = random_stencil_net(2)
    si = net[4]
    rng = np.random.default_rng(nz * 1000 + ncol)
    fields = [rng.uniform(si[i, 0], si[i, 1], shape) for i in range(5)]
    check_against_restatement(fields, nz, net, shape)


@pytest.mark.parametrize("feature", range(9))
def test_stencil_operand_layout_one_hot(mw, feature):
    """W1 with a single 1 in row `feature`: the output is that feature alone -- the right FIELD of the right LEVEL (k for features 0..4,
    min(nz - 1, k + 1) for 5..8: the top level reads itself).  Exact small numbers, identity scaling: both kernels give the value itself.
    nz = 22 runs in three z chunks (8, 8, 6), so the carried level crosses chunk borders of both parities."""
    from miniweatherml_amd import capi
    nz, ncol = 22, 45
    assert capi.lib().mw_mlp_stencil_chunk(nz, ncol) == 8
    rng = np.random.default_rng(feature)
    fields = [rng.integers(1, 9, (nz, ncol)).astype(np.float64) / 8.0 + v for v in range(5)]       # field v lies in (v, v + 1]
    u, n = (3 * feature + 1) % 10, feature % 4
    W1, W2 = np.zeros((9, 10), np.float32), np.zeros((10, 4), np.float32)
    W1[feature, u] = 1.0
    W2[u, n] = 1.0
    ident9, ident4 = np.ascontiguousarray([[0., 1.]] * 9), np.ascontiguousarray([[0., 1.]] * 4)
    net = (W1, np.zeros(10, np.float32), W2, np.zeros(4, np.float32), ident9, ident4)
    src = fields[(0, 1, 2, 3, 4, 0, 2, 3, 4)[feature]]
    if feature >= 5:
        src = src[np.minimum(np.arange(nz) + 1, nz - 1)]
        assert np.array_equal(src[nz - 1], fields[(0, 2, 3, 4)[feature - 5]][nz - 1]) and not np.array_equal(src[0], src[1])
    for outs in run_both(fields, nz, net):
        for o in range(4):
            assert np.array_equal(outs[o].reshape(nz, ncol), src if o == n else np.zeros((nz, ncol))), (feature, o)


def test_stencil_with_dead_rows_is_the_single_cell_model(mw, oracle):
    """Rows 5..8 of W1 zero, the rest the shipped single-cell weights: strict equals mlp_forward's strict form, production its MFMA form
    within the MLP tolerance."""
    import torch
    from miniweatherml_amd import modules
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    net9 = (np.ascontiguousarray(np.concatenate([W1, np.zeros((4, 10), np.float32)])), b1, W2, b2,
            np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]])), so)
    f = rainy_state(oracle, 20, 16, 24)
    fields = [f.temp, f.rho_d, f.tracers[0], f.tracers[1], f.tracers[2]]
    strict9, fast9 = run_both(fields, 24, net9)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in fields]
    strict5 = [o.cpu().numpy().ravel() for o in modules.mlp_forward(*t, W1, b1, W2, b2, si, so, strict=1)]
    fast5 = [o.cpu().numpy().ravel() for o in modules.mlp_forward(*t, W1, b1, W2, b2, si, so)]
    for n in range(4):
        assert np.array_equal(strict9[n], strict5[n]), n
        assert np.max(np.abs(fast9[n] - fast5[n])) <= mlp_tol(so, n), n
        assert np.max(np.abs(fast9[n] - strict5[n])) <= mlp_tol(so, n), n


def test_stencil_forward_refuses_in_place(mw):
    import torch
    from miniweatherml_amd import modules
    from miniweatherml_amd.capi import MWError
    net = random_stencil_net(4)
    t = [torch.rand(4, 20, dtype=torch.float64, device="cuda") for _ in range(5)]
    with pytest.raises(MWError, match="must not overlap"):
        modules.mlp_stencil_forward(4, *t, *net, outs=[t[0], torch.empty_like(t[0]), torch.empty_like(t[0]), torch.empty_like(t[0])])


def test_ponni_forward_nine_input_stack_on_the_mfma_path(mw):
    """mw_ponni_forward gives the 9 -> 10 -> 4 stack the MFMA tiles (the trainer's validation pass): within 1e-5 of the strict form."""
    import torch
    from miniweatherml_amd import modules
    W1, b1, W2, b2, _, _ = random_stencil_net(5)
    layers = [("matvec", W1), ("bias", b1), ("relu", 10, 0.1), ("matvec", W2), ("bias", b2)]
    for batch in (1, 17, 1000, 4099):
        x = torch.rand((9, batch), dtype=torch.float32, device="cuda") * 1.4 - 0.2
        ref = modules.ponni_forward(layers, x, strict=1).cpu().numpy()
        out = modules.ponni_forward(layers, x).cpu().numpy()
        assert out.shape == (4, batch) and np.max(np.abs(out - ref)) <= 1e-5
        xs = x.cpu().numpy().astype(np.float64)
        pre = xs.T @ W1.astype(np.float64) + b1
        ref64 = (np.where(pre > 0, pre, 0.1 * pre) @ W2.astype(np.float64) + b2).T
        assert np.max(np.abs(out - ref64)) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
def C_ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def to_file_layout(x9):
    """(n, 9) features -> DataGenerator's inputs (n, 5, 2); the never-assigned [4, 1] entry gets a value of its own."""
    ins = np.full((x9.shape[0], 5, 2), 7.0, np.float32)
    ins[:, :, 0] = x9[:, :5]
    ins[:, 0:4, 1] = x9[:, 5:]
    return ins


def kessler_like9(n, seed):
    """Synthetic stencil samples with Kessler-like ranges: the single-cell map of tests/test_gpu_surrogate_train.py plus rain falling in
    from the level above."""
    rng = np.random.default_rng(seed)
    lo = np.array([200.0, 0.1, 0.0, 0.0, 0.0, 195.0, 0.0, 0.0, 0.0])
    hi = np.array([300.0, 1.2, 0.02, 0.004, 0.015, 295.0, 0.018, 0.004, 0.015])
    x = lo + (hi - lo) * rng.random((n, 9))
    conv = 0.3 * x[:, 3] * (1.0 + np.tanh((x[:, 0] - 250.0) / 20.0))
    y = np.stack([x[:, 0] + 400.0 * conv + 0.02 * (x[:, 5] - x[:, 0]), x[:, 2] + 0.2 * conv * x[:, 1], x[:, 3] - conv + 0.1 * x[:, 7],
                  0.6 * x[:, 4] + 0.4 * x[:, 8] + 0.8 * conv], axis=1)
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("batch", GRAD_BATCHES)
def test_stencil_batch_gradient_matches_torch_autograd(mw, batch):
    """The batch sizes and the assertions of tests/test_gpu_surrogate_train.py::test_batch_gradient_matches_torch_autograd."""
    import torch
    from miniweatherml_amd import capi
    w, x, y = gradient_case(9, batch)
    g, loss_v = device_batch_grad(9, w, x, y)
    dev = [torch.from_numpy(a).cuda() for a in (w, x, y)]
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    P = torch_model(w)
    xt = torch.tensor(x.T.astype(np.float64))
    assert signs_ok(9, w, x)
    ref = torch.nn.functional.mse_loss(torch_forward(P, xt), torch.tensor(y.T.astype(np.float64)))
    ref.backward()
    g_ref = np.concatenate([p.grad.numpy().ravel() for p in P])
    assert np.all(g_ref != 0.0)                                       # every one of the 144 entries is exercised
    print("batch %d: max|dg|/max|g| %.2e" % (batch, np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref))))
    assert np.max(np.abs(g - g_ref)) <= 1e-5 * np.max(np.abs(g_ref)), np.max(np.abs(g - g_ref)) / np.max(np.abs(g_ref))
    assert abs(loss_v - float(ref.detach())) <= 1e-6 * float(ref.detach())
    check_rho(9, w, x, y, g, "stencil, batch %d" % batch)
    # the v2 entry with n_in = 5 is the single-cell routine
    g5a, g5b = torch.empty(104, dtype=torch.float32, device="cuda"), torch.empty(104, dtype=torch.float32, device="cuda")
    d5 = [dev[0][:104].contiguous(), dev[1][:5].contiguous(), dev[2]]
    capi.check(capi.lib().mw_surrogate_batch_grad_v2(5, *[C_ptr(t) for t in d5], batch, C_ptr(g5a), C_ptr(loss), None))
    capi.check(capi.lib().mw_surrogate_batch_grad(*[C_ptr(t) for t in d5], batch, C_ptr(g5b), C_ptr(loss), None))
    assert torch.equal(g5a, g5b)


@pytest.fixture(scope="module")
def file20k(tmp_path_factory):
    x9, outs = kessler_like9(20000, 1)
    ins = to_file_layout(x9)
    return write_sample_file(tmp_path_factory.mktemp("s20k9") / "s.nc", [(ins[:7000], outs[:7000]), (ins[7000:], outs[7000:])]), x9, outs


# max|dw| / max|w|, then loss, val_loss, mean_absolute_error, val_mean_absolute_error (largest relative deviation over the epochs).
# Measured on the MI355X with the bias correction of surrogate_train.kernel_nadam_table: 2.23e-7, 5.70e-8, 1.97e-8, 2.21e-8, 1.20e-8;
# bounds = 3 x measured, rounded up to one digit (before: 3.2e-6, 1.2e-6, 2.4e-6 under the bounds 1e-5, 4e-6, 8e-6).  torch's fp32 replay
# on the CPU deviates from the fp64 one by 3.0e-7, 3.3e-9, 1.6e-7, 4.0e-8, 1.0e-7.
TRAJECTORY_BOUNDS = (7e-7, 2e-7, 6e-8)
MAE_BOUNDS = (7e-8, 4e-8)


def test_stencil_two_epoch_trajectory_matches_torch_nadam(mw, file20k):
    """2 epochs on 20,000 stencil samples at batch 1024 (13 steps per epoch, the last one partial) from the product's seeded initial
    weights in the product's batch order, against torch fp64 NAdam(eps=1e-7, momentum_decay=4e-3).  Measured values and bounds: TRAJECTORY_BOUNDS,
    MAE_BOUNDS above."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    path, x9, outs = file20k
    seed = 5
    r = st.train_surrogate([path], epochs=2, batch_size=1024, seed=seed, stencil=True)
    assert r["inputs"] == "stencil" and r["weights"].shape == (1, 144)
    (tx, ty), (vx, vy), _ = host_sets(x9, outs, seed)
    assert (r["n_train"], r["n_val"], r["n_test"]) == (12800, 3200, 4000) and tx.shape == (12800, 9)
    w_ref, h_ref = replay(torch.float64, [(tx, ty), (vx, vy)], seed, 1024, 2, 1e-3, stencil=True)
    w = r["weights"][0].astype(np.float64)
    dw, dl, dm, dv, dvm = deviations(w, r["history"][0], w_ref, h_ref)
    print("stencil trajectory: max|dw|/max|w| %.2e, loss %.2e, val_loss %.2e, mean_absolute_error %.2e, val_mean_absolute_error %.2e"
          % (dw, dl, dv, dm, dvm))
    assert dw <= TRAJECTORY_BOUNDS[0] and dl <= TRAJECTORY_BOUNDS[1] and dv <= TRAJECTORY_BOUNDS[2]
    assert dm <= MAE_BOUNDS[0] and dvm <= MAE_BOUNDS[1]
    assert np.max(np.abs(w - st.initial_weights(seed, 1, stencil=True)[0])) > 5e-3      # it moved
    assert np.max(np.abs(w[50:90] - st.initial_weights(seed, 1, stencil=True)[0][50:90])) > 1e-3   # so did the level-above rows of W1


def test_stencil_training_is_deterministic_and_models_independent(mw, file20k):
    """Run-to-run identity; model m of a K = 4 run is bitwise the K = 1 run of seed + m on the same split."""
    from miniweatherml_amd import surrogate_train as st
    a = st.train_surrogate([file20k[0]], epochs=2, batch_size=512, seed=3, models=2, stencil=True)
    b = st.train_surrogate([file20k[0]], epochs=2, batch_size=512, seed=3, models=2, stencil=True)
    assert np.array_equal(a["weights"].view(np.uint32), b["weights"].view(np.uint32))
    assert a["history"] == b["history"] and a["test_metrics"] == b["test_metrics"]
    r4 = st.train_surrogate([file20k[0]], epochs=2, batch_size=1000, seed=10, models=4, stencil=True)
    assert r4["seeds"] == [10, 11, 12, 13] and r4["split_seed"] == 10 and r4["weights"].shape == (4, 144)
    for m in (0, 2):
        r1 = st.train_surrogate([file20k[0]], epochs=2, batch_size=1000, seed=10 + m, models=1, split_seed=10, stencil=True)
        assert np.array_equal(r1["weights"][0].view(np.uint32), r4["weights"][m].view(np.uint32))
        assert r1["history"][0] == r4["history"][m]
    final = [h["val_loss"][-1] for h in r4["history"]]
    assert r4["best_model"] == int(np.argmin(final)) and len(set(final)) == 4


def test_stencil_inputs_reach_the_network(mw, tmp_path):
    """A target that only the stencil model can fit: 20,000 samples, nine features i.i.d. uniform [0, 1), outputs (x0, x2, x3, 0.5 x4 +
    0.5 x8).  x8 is independent of everything the single-cell model sees, so its validation loss cannot go below floor = var(0.5 x8) / 4
    (of the min-max-scaled target, on the validation rows).  Torch fp64 with the same optimizer and init range reached 1.8e-4 .. 3.9e-4
    with nine features over four seeds and 5.2e-3 .. 5.7e-3 with five.  Asserted: stencil < floor / 4, single cell > floor / 2."""
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(3)
    x = rng.random((20000, 9))
    y = np.stack([x[:, 0], x[:, 2], x[:, 3], 0.5 * x[:, 4] + 0.5 * x[:, 8]], axis=1)
    x32, y32 = x.astype(np.float32), y.astype(np.float32)
    path = write_sample_file(tmp_path / "u.nc", [(to_file_layout(x32), y32)])
    n_train, n_val, _ = st.split_sizes(20000)
    val_rows = st.preshuffle_permutation(20000, 0)[n_train:n_train + n_val]
    rng3 = float(y32[:, 3].max()) - float(y32[:, 3].min())
    floor = float(np.var(0.5 * x32[val_rows, 8].astype(np.float64) / rng3)) / 4.0
    assert 4.5e-3 < floor < 6e-3
    kw = dict(epochs=20, batch_size=128, learning_rate=1e-2, seed=0)
    r9 = st.train_surrogate([path], stencil=True, **kw)
    r5 = st.train_surrogate([path], **kw)
    v9, v5 = r9["history"][0]["val_loss"][-1], r5["history"][0]["val_loss"][-1]
    print("floor %.3e: stencil val_loss %.3e (floor / %.1f), single-cell val_loss %.3e (%.2f floor)" % (floor, v9, floor / v9, v5, v5 / floor))
    assert v9 < floor / 4
    assert v5 > floor / 2


def rainy_samples(oracle, tmp_path, nx, ny, nz):
    """DataGenerator's file of EVERY cell of a rainy supercell state before / after the GPU Kessler; returns the generator, the input
    coupler, the oracle state it was pushed from, and dt."""
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
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
    assert gen.generate_samples_stencil(inp, coupler, dt, 0.0, seed=1) == nx * ny * nz
    return gen, inp, f, dt


def test_stencil_cli_then_inference_ponni_driver(mw, oracle, tmp_path, monkeypatch, capsys):
    """python -m miniweatherml_amd.surrogate_train FILES --stencil --out DIR, then driver inference_ponni with keras_weights_txt /
    nn_input_scaling pointing into DIR: no new YAML key; the module runs the stencil network."""
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver, microphysics, surrogate_train as st
    from util import gpu_fields
    gen, _, _, _ = rainy_samples(oracle, tmp_path, 32, 32, 16)
    monkeypatch.chdir(tmp_path)
    assert st.main([gen.fname, "--stencil", "--out", "trained", "--epochs", "2", "--batch-size", "256"]) == 0
    assert "wrote" in capsys.readouterr().out and len(np.loadtxt("trained/weights.txt", comments="#")) == 144
    seen = []
    real = microphysics.mlp_stencil_forward                              # where Microphysics_Kessler_Surrogate.time_step looks the name up
    monkeypatch.setattr(microphysics, "mlp_stencil_forward", lambda *a, **k: (seen.append(a[6].shape), real(*a, **k))[1])
    path, _ = write_yaml(tmp_path, nx=32, ny=1, nz=20, xlen=32000., extra='keras_weights_txt: "trained/weights.txt"\n'
                         'nn_input_scaling: "trained/input_scaling.txt"\nnn_output_scaling: "trained/output_scaling.txt"')
    coupler, dycore, info = driver.run("inference_ponni", path, max_steps=3, quiet=True)
    assert info["steps"] == 3 and np.isfinite(gpu_fields(coupler)["temp"]).all()
    assert seen == [(9, 10)] * 3


def test_stencil_generate_train_infer_end_to_end(mw, oracle, tmp_path):
    """Every cell of a rainy supercell state after the GPU Kessler (131,072 samples) -> generate_samples_stencil -> train_surrogate(stencil
    =True), 10 epochs at batch 256 -> files -> load_surrogate_weights -> mlp_stencil_forward on the input coupler against the restatement;
    one online step of Microphysics_Kessler_Surrogate leaves exactly the network's outputs in the four fields.  Asserted: the project's
    bound for this data, val_loss <= variance baseline / 20.  The stencil and single-cell val_loss are printed."""
    import torch
    from miniweatherml_amd import modules, surrogate_train as st
    from util import gpu_fields
    nx, ny, nz = 64, 64, 32
    gen, inp, f, dt = rainy_samples(oracle, tmp_path, nx, ny, nz)
    # the file's nine columns are the host statement of the feature order on the input state (samples are in cell order)
    g = gpu_fields(inp)
    fields = [g["temp"], g["density_dry"], g["tracer0"], g["tracer1"], g["tracer2"]]
    x9, y4, _ = st.read_samples([gen.fname], stencil=True)
    assert np.array_equal(x9, modules.stencil_features(fields, nz).T.astype(np.float32))
    out_dir = str(tmp_path / "trained")
    r = st.train_surrogate([gen.fname], out_dir=out_dir, epochs=10, batch_size=256, seed=0, stencil=True)
    r5 = st.train_surrogate([gen.fname], epochs=10, batch_size=256, seed=0)
    (tx, ty), _, test_set = host_sets(x9, y4, 0)
    check_test_metrics(r, test_set, "stencil end to end")
    baseline = float(np.mean(np.var(ty.astype(np.float64), axis=0)))
    v9, v5 = r["history"][0]["val_loss"][-1], r5["history"][0]["val_loss"][-1]
    print("variance baseline %.3e: stencil val_loss %.3e (1/%.0f), single-cell val_loss %.3e (1/%.0f), stencil / single %.3f"
          % (baseline, v9, baseline / v9, v5, baseline / v5, v9 / v5))
    assert v9 <= baseline / 20
    hist = json.load(open(os.path.join(out_dir, "history.json")))
    assert hist["inputs"] == "stencil" and hist["best_model"] == 0
    paths = [os.path.join(out_dir, p) for p in ("weights.txt", "input_scaling.txt", "output_scaling.txt")]
    net = modules.load_surrogate_weights(weights_txt=paths[0], in_scaling_txt=paths[1], out_scaling_txt=paths[2])
    assert net[0].shape == (9, 10) and np.array_equal(np.concatenate([net[0].ravel(), net[1], net[2].ravel(), net[3]]), r["weights"][0])
    so = net[5]
    dm = inp.get_data_manager_readwrite()
    outs = modules.mlp_stencil_forward(nz, *[dm.get(n) for n in FIELDS], *net)
    ref = np_stencil_forward(fields, nz, *net)
    for k in range(4):
        assert np.max(np.abs(outs[k].cpu().numpy().ravel() - ref[k])) <= mlp_tol(so, k), k
    # the model in the loop: the module picks the stencil kernel from the files, and `online` writes its outputs back
    sur = modules.Microphysics_Kessler_Surrogate()
    init = sur.init
    sur.init = lambda c: init(c, weights_txt=paths[0], in_scaling_txt=paths[1], out_scaling_txt=paths[2])      # what the driver passes
    c2, _, sur = modules.make_supercell(nx, ny, nz, 1, 500.0 * nx, 500.0 * ny, 20000., micro=sur)
    push_fields(c2, f)
    assert sur.W1.shape == (9, 10) and all(torch.equal(c2.get_data_manager_readonly().get(n, True), dm.get(n, True)) for n in FIELDS)
    sur.online = True
    nn = sur.time_step(c2, dt)
    dm2 = c2.get_data_manager_readonly()
    for k, name in enumerate(("temp", "water_vapor", "cloud_liquid", "precip_liquid")):
        got = dm2.get(name, True)
        assert torch.equal(got, nn[k]) and torch.equal(got, outs[k]), name
    assert set(sur._diffs) == {"rho_v", "rho_c", "rho_r", "temp"} and all(np.isfinite(v) for v in sur._diffs.values())
    assert torch.equal(dm2.get("density_dry", True), dm.get("density_dry", True))
    sur.mlp_strict = 1
    push_fields(c2, f)
    nn1 = sur.time_step(c2, dt)
    for k in range(4):
        assert np.array_equal(nn1[k].cpu().numpy().ravel(), ref[k]), k
