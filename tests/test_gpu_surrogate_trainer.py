"""The surrogate trainer's kernels one by one (csrc/mw_train.hip) against the yardsticks of tests/surrogate_ref.py, on the MI355X:
k_surrogate_prepare bit for bit, k_surrogate_sums / k_surrogate_sums_final against extended precision, the batch gradient where its
sums cancel, and everything train_surrogate reports at the edge configurations of the batch loop.

Trajectory deviations against the torch fp64 replay (surrogate_ref.replay), MEASURED on the MI355X on the first run with the mended Nadam table; bound = 3 x measured,
rounded up to one digit (BOUNDS below); `fp32 replay` = the same replay in torch fp32 on the CPU against the fp64 one.  Columns:
max|dw| / max|w|, then the largest relative deviation of loss, mean_absolute_error, val_loss, val_mean_absolute_error over the epochs.

configuration             max|dw|  loss     mae      val_loss val_mae
(a) single   measured    3.82e-06 3.61e-08 1.95e-08 1.29e-07 5.72e-08
             bound       2e-05    2e-07    6e-08    4e-07    2e-07
             fp32 replay 5.3e-06  5.8e-08  3.3e-08  1.3e-07  4.4e-08
             before fix  1.07e-05 2.74e-06 1.40e-06 5.95e-07 3.15e-07
(b) single   measured    6.71e-08 8.90e-08 6.89e-08 1.86e-10 1.27e-10
             bound       3e-07    3e-07    3e-07    6e-10    4e-10
             fp32 replay 8.5e-08  1.1e-07  3.7e-08  8.9e-08  9.8e-08
             before fix  2.82e-07 8.90e-08 6.89e-08 6.13e-08 3.96e-08
(c) single   measured    8.20e-08 3.42e-08 2.73e-07 1.86e-10 1.11e-10
             bound       3e-07    2e-07    9e-07    6e-10    4e-10
             fp32 replay 1.4e-07  6.5e-08  3.8e-08  1.0e-07  2.7e-08
             before fix  5.12e-07 6.79e-08 2.88e-07 1.14e-07 7.52e-08
(d) single   measured    2.85e-07 2.43e-08 1.42e-08 2.67e-08 1.40e-08
             bound       9e-07    8e-08    5e-08    9e-08    5e-08
             fp32 replay 3.2e-07  2.5e-08  2.2e-08  1.0e-07  1.4e-07
             before fix  3.87e-06 4.43e-06 2.57e-06 7.60e-06 3.83e-06
(e) single   measured    5.11e-07 6.88e-08 2.70e-08 4.11e-07 1.77e-07
             bound       2e-06    3e-07    9e-08    2e-06    6e-07
             fp32 replay 4.0e-07  2.5e-07  1.3e-07  4.3e-07  2.9e-07
             before fix  1.31e-05 7.57e-06 4.30e-06 2.44e-05 1.26e-05
(a) stencil  measured    6.32e-07 3.81e-08 2.16e-08 7.19e-08 2.74e-08
             bound       2e-06    2e-07    7e-08    3e-07    9e-08
             fp32 replay 1.3e-06  2.5e-08  1.0e-08  5.1e-08  7.5e-08
             before fix  2.42e-06 2.66e-06 1.47e-06 2.05e-07 4.36e-08
(c) stencil  measured    8.92e-08 2.52e-07 3.76e-07 8.04e-10 5.89e-10
             bound       3e-07    8e-07    2e-06    3e-09    2e-09
             fp32 replay 1.4e-07  5.3e-08  4.3e-08  9.5e-08  4.9e-08
             before fix  5.58e-07 2.52e-07 4.60e-07 1.24e-07 7.95e-08
(d) stencil  measured    3.09e-07 7.77e-08 2.64e-08 1.07e-07 5.60e-08
             bound       1e-06    3e-07    8e-08    4e-07    2e-07
             fp32 replay 3.7e-07  7.4e-08  4.6e-08  2.1e-07  5.5e-08
             before fix  3.91e-06 6.80e-06 3.96e-06 1.05e-05 5.11e-06

`before fix` = the same run with the bias correction built from beta2 = 0.999 instead of the kernel's fp32(0.999) (surrogate_train.
kernel_nadam_table): this test caught it -- configurations (d) and (e) then miss every bound, most by a factor above 10.
"""
import ctypes

import numpy as np
import pytest

import surrogate_ref as sr
from test_surrogate_train_cpu import write_sample_file

pytestmark = pytest.mark.gpu

BOUNDS = {('a', False): (2e-05, 2e-07, 6e-08, 4e-07, 2e-07),
          ('b', False): (3e-07, 3e-07, 3e-07, 6e-10, 4e-10),
          ('c', False): (3e-07, 2e-07, 9e-07, 6e-10, 4e-10),
          ('d', False): (9e-07, 8e-08, 5e-08, 9e-08, 5e-08),
          ('e', False): (2e-06, 3e-07, 9e-08, 2e-06, 6e-07),
          ('a', True): (2e-06, 2e-07, 7e-08, 3e-07, 9e-08),
          ('c', True): (3e-07, 8e-07, 2e-06, 3e-09, 2e-09),
          ('d', True): (1e-06, 3e-07, 8e-08, 4e-07, 2e-07),}                                                            # (configuration, stencil) -> (dw, loss, mae, val_loss, val_mae)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
# k_surrogate_prepare
def device_prepare(n_in, raw_in, raw_out, scl_in, scl_out, seed, n_train, n_val):
    """mw_surrogate_prepare_v2 on host arrays; returns the six output arrays (train x, y, val x, y, test x, y), feature-major fp32."""
    import torch
    from miniweatherml_amd import capi
    n = raw_in.shape[0]
    dev_in, dev_out = torch.from_numpy(np.ascontiguousarray(raw_in)).cuda(), torch.from_numpy(np.ascontiguousarray(raw_out)).cuda()
    sizes = [(rows, max(k, 0)) for k in (n_train, n_val, n - n_train - n_val) for rows in (n_in, 4)]
    outs = [torch.full((max(rows * k, 1),), float("nan"), dtype=torch.float32, device="cuda") for rows, k in sizes]     # never a null pointer
    dp = ctypes.POINTER(ctypes.c_double)
    si, so = np.ascontiguousarray(scl_in, np.float64), np.ascontiguousarray(scl_out, np.float64)
    assert si.shape == (n_in, 2) and so.shape == (4, 2)
    capi.check(capi.lib().mw_surrogate_prepare_v2(n_in, n, ptr(dev_in), ptr(dev_out), si.ctypes.data_as(dp), so.ctypes.data_as(dp), seed,
                                                  n_train, n_val, *[ptr(t) for t in outs], None))
    torch.cuda.synchronize()
    return [t.cpu().numpy()[:rows * k].reshape(rows, k) for t, (rows, k) in zip(outs, sizes)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n_in", [5, 9])
@pytest.mark.parametrize("case", sr.prepare_cases(), ids=lambda c: "n%d-test%g-val%g" % c)
def test_prepare_is_bitwise_the_host_statement(mw, n_in, case):
    """Every element of the six arrays: fp64 subtract, fp64 divide and the fp64 -> fp32 conversion are correctly rounded on both sides
    (the build has no fast-math), so anything short of bit equality is a finding.  The sizes sit around the Feistel domain's powers of
    four; the last one runs the kernel's grid-stride loop (n > 4096 blocks x 256 threads)."""
    from miniweatherml_amd import surrogate_train as st
    n, ts, vs = case
    seed = 11 + n
    x, y = sr.raw_samples(n, n_in, seed)
    scl_in, scl_out = st.data_scaling(x, y)
    n_train, n_val, n_test = st.split_sizes(n, ts, vs)
    got = device_prepare(n_in, x, y, scl_in, scl_out, seed, n_train, n_val)
    want = [a.T for pair in sr.host_sets(x, y, seed, ts, vs) for a in pair]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.shape[1] == (n_train, n_val, n_test)[k // 2]
        assert np.array_equal(bits(g), bits(w)), (k, int(np.sum(bits(g) != bits(w))), np.argwhere(bits(g) != bits(w))[:3])


@pytest.mark.parametrize("seed", [0, 5, 2 ** 63 + 1])
def test_prepare_applies_the_preshuffle_permutation(mw, seed):
    """Identity scaling (min 0, max 1) and the sample's own index in column 0 (exact in fp32 below 2^24): the outputs ARE the device's
    pre-shuffle.  It equals preshuffle_permutation(n, seed) and is a bijection of [0, n)."""
    from miniweatherml_amd import surrogate_train as st
    ident = lambda rows: np.array([[0.0, 1.0]] * rows)                 # noqa: E731
    for n in sr.PREPARE_SIZES:
        for n_in in (5, 9):
            rng = np.random.default_rng(n)
            x = rng.random((n, n_in), dtype=np.float32)
            y = rng.random((n, 4), dtype=np.float32)
            x[:, 0] = np.arange(n)
            y[:, 3] = np.arange(n)
            n_train, n_val, _ = st.split_sizes(n)
            got = device_prepare(n_in, x, y, ident(n_in), ident(4), seed, n_train, n_val)
            perm = st.preshuffle_permutation(n, seed)
            dev = np.concatenate([got[0][0], got[2][0], got[4][0]]).astype(np.int64)
            assert np.array_equal(dev, perm), (n, n_in)
            assert np.array_equal(np.sort(dev), np.arange(n)), (n, n_in)
            assert np.array_equal(np.concatenate([got[1][3], got[3][3], got[5][3]]).astype(np.int64), perm)       # x and y of the same sample
            for f in range(1, n_in):                                                                               # every other column moved with it
                assert np.array_equal(np.concatenate([got[0][f], got[2][f], got[4][f]]), x[perm, f]), (n, n_in, f)
            if n > 16:
                assert not np.array_equal(dev, np.arange(n))


def test_prepare_refusals(mw):
    from miniweatherml_amd import surrogate_train as st
    from miniweatherml_amd.capi import MWError
    n = 100
    for n_in in (5, 9):
        x, y = sr.raw_samples(n, n_in, 1)
        scl_in, scl_out = st.data_scaling(x, y)
        for row in range(n_in + 4):
            for hi in ("equal", "below"):
                si, so = scl_in.copy(), scl_out.copy()
                tab, r = (si, row) if row < n_in else (so, row - n_in)
                tab[r, 1] = tab[r, 0] if hi == "equal" else tab[r, 0] - 1.0
                with pytest.raises(MWError, match=r"%s %d has max <= min" % ("input" if row < n_in else "output", r)):
                    device_prepare(n_in, x, y, si, so, 0, 64, 16)
        for n_train, n_val in ((0, 16), (64, 0), (64, 36), (100, 0), (0, 0)):
            with pytest.raises(MWError, match="every set needs at least one sample"):
                device_prepare(n_in, x, y, scl_in, scl_out, 0, n_train, n_val)
        assert len(device_prepare(n_in, x, y, scl_in, scl_out, 0, 64, 35)[4][0]) == 1       # the smallest test set is accepted


# ---------------------------------------------------------------------------------------------------------------------------------
# k_surrogate_sums, k_surrogate_sums_final
def device_errors(pred, y):
    """mw_surrogate_errors on pred (nsets, 4, n), y (4, n) fp32: (nsets, 4, 6) fp64."""
    import torch
    from miniweatherml_amd import capi
    nsets, _, n = pred.shape
    L = capi.lib()
    dp, dy = torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda()
    ws = torch.empty(int(L.mw_surrogate_errors_workspace_bytes(nsets)), dtype=torch.uint8, device="cuda")
    out = torch.full((nsets, 24), float("nan"), dtype=torch.float64, device="cuda")
    capi.check(L.mw_surrogate_errors(n, nsets, ptr(dp), ptr(dy), ptr(ws), ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nsets, 4, 6)


@pytest.mark.parametrize("nsets", sr.ERROR_NSETS)
@pytest.mark.parametrize("n", sr.ERROR_SIZES)
def test_error_sums_against_extended_precision(mw, n, nsets):
    """The maxima are exact.  Every sum is within n 2^-52 sum|x_i| of the exact one: the bound of an n-term fp64 sum in ANY order, so the
    kernel's order (grid-stride per thread, a tree per block, 128 partials in sequence) needs no measurement.  Each set's 24 numbers come
    from that set's predictions (nsets = 1, 3, 5 leave k_surrogate_sums_final's last block half empty)."""
    pred, y = sr.errors_case(n, nsets)
    got = device_errors(pred, y)
    worst = 0.0
    for s in range(nsets):
        stats, mass = sr.error_sums_ref(pred[s], y)
        assert np.array_equal(got[s][:, 4:], stats[:, 4:]), (s, got[s][:, 4:], stats[:, 4:])
        err, bound = np.abs(got[s][:, :4] - stats[:, :4]), n * 2.0 ** -52 * mass
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (s, err / bound)
    print("n %d, %d sets: worst |sum - exact| / (n 2^-52 sum|x|) = %.2e" % (n, nsets, worst))
    for a in range(nsets):
        for b in range(a):
            assert np.all(got[a][:, :3] != got[b][:, :3]) and got[a][1, 4] != got[b][1, 4], (a, b)
            assert np.array_equal(got[a][:, 3], got[b][:, 3]) and np.array_equal(got[a][:, 5], got[b][:, 5])      # the targets are shared


# ---------------------------------------------------------------------------------------------------------------------------------
# the batch gradient where its sums cancel
@pytest.mark.parametrize("n_in", [5, 9])
@pytest.mark.parametrize("batch", sr.NEAR_FIT_BATCHES)
def test_batch_gradient_near_a_fit(mw, n_in, batch):
    """Targets = the network's fp64 output + 1e-2 N(0, 1): centred residuals, every entry a cancelling sum (at least half with
    T_e / |g_e| >= 10).  max|dg| / max|g| means nothing here (plain fp32 on the CPU reaches 4.5e-4): the per-entry rho and the loss."""
    w, x, y = sr.near_fit_case(n_in, batch)
    assert sr.signs_ok(n_in, w, x)
    g_ref, T, loss_ref, _ = sr.grad_summary(sr.grad_terms(n_in, w, x.T, y.T))
    assert np.mean(T >= 10 * np.abs(g_ref)) >= 0.5
    g, loss = sr.device_batch_grad(n_in, w, x, y)
    sr.check_rho(n_in, w, x, y, g, "near fit, n_in %d, batch %d" % (n_in, batch))
    assert abs(loss - loss_ref) <= 1e-6 * loss_ref, abs(loss - loss_ref) / loss_ref


# ---------------------------------------------------------------------------------------------------------------------------------
# everything train_surrogate reports, at the edge configurations
def configuration_samples(name, stencil):
    """(inputs in the file's layout (n, 5, 2), the model's features (n, 5 | 9), outputs (n, 4)) of a configuration."""
    from test_gpu_surrogate_stencil import kessler_like9, to_file_layout
    from test_gpu_surrogate_train import kessler_like
    n = sr.CONFIGS[name]["n"]
    if stencil:
        x9, outs = kessler_like9(n, ord(name))
        return to_file_layout(x9), x9, outs
    ins, outs = kessler_like(n, ord(name))
    return ins, np.ascontiguousarray(ins[:, :, 0]), outs


@pytest.mark.parametrize("name,stencil", sr.CONFIG_CASES, ids=lambda v: v if isinstance(v, str) else ("stencil" if v else "single"))
def test_reports_at_the_edge_configurations(mw, tmp_path, name, stencil):
    """(a) batch 1: 256 steps with one live lane.  (b) a training set of 640 below the batch of 1024: one step per epoch.  (c) the largest
    batch, 8192 + 4608.  (d) 3200 = 32 x 100: the last batch is full, so the batch routine ends without a prefetch.  (e) 50 steps of 257
    at learning rate 1e-2.  Weights and all four history series against the fp64 replay (bounds: the table at the top), test_metrics and
    test_loss against the fp64 forward of the final weights."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    c = sr.CONFIGS[name]
    ins, feats, outs = configuration_samples(name, stencil)
    path = write_sample_file(tmp_path / "s.nc", [(ins, outs)])
    r = st.train_surrogate([path], epochs=c["epochs"], batch_size=c["batch"], learning_rate=c["lr"], seed=sr.CONFIG_SEED, stencil=stencil)
    assert (r["n_train"], r["n_val"], r["n_test"]) == c["split"] and r["weights"].shape == (1, sr.n_par(9 if stencil else 5))
    sets = sr.host_sets(feats, outs, sr.CONFIG_SEED)
    w_ref, h_ref = sr.replay(torch.float64, sets, sr.CONFIG_SEED, c["batch"], c["epochs"], c["lr"], stencil)
    h = r["history"][0]
    assert all(len(h[k]) == c["epochs"] for k in sr.SERIES)
    dev = sr.deviations(r["weights"][0], h, w_ref, h_ref)
    print("TRAJECTORY %s %s: dw %.2e loss %.2e mae %.2e val_loss %.2e val_mae %.2e" % ((name, "stencil" if stencil else "single") + dev))
    sr.check_test_metrics(r, sets[2], "(%s)" % name)
    assert np.max(np.abs(r["weights"][0] - st.initial_weights(sr.CONFIG_SEED, 1, stencil=stencil)[0])) > 1e-3          # it moved
    assert all(d <= b for d, b in zip(dev, BOUNDS[name, stencil])), (dev, BOUNDS[name, stencil])


@pytest.mark.parametrize("stencil", [False, True], ids=["single", "stencil"])
def test_validation_in_smaller_prediction_groups(mw, stencil):
    """Trainer.validate when the models do not fit one prediction group: three models validated in groups of 2 + 1 and 1 + 1 + 1 (the
    g0 offset into vstats, k_surrogate_sums_final with one set) leave bitwise the sums of the default single group of three."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    ins, feats, outs = configuration_samples("d", stencil)
    scl_in, scl_out = st.data_scaling(feats, outs)
    split = st.split_sizes(len(feats))

    def run(group):
        tr = st.Trainer(torch.from_numpy(feats).cuda(), torch.from_numpy(outs).cuda(), scl_in, scl_out, split, seed=3, models=3,
                        batch_size=128, epochs=1)
        assert tr.group == 3
        if group is not None:
            tr.group = group
        w, ts, _ = tr.epoch()
        w2, ts2, vs = tr.finish()
        assert np.array_equal(w, w2) and np.array_equal(ts, ts2)
        return w, ts, vs

    w3, ts3, vs3 = run(None)
    assert np.all(np.isfinite(vs3)) and np.all(vs3[:, 0] > 0) and len({vs3[m, 0] for m in range(3)}) == 3
    sets = sr.host_sets(feats, outs, 3)
    for m in range(3):                                                 # and they are each model's own validation sums
        stats, _ = sr.error_sums_ref(sr.forward64(w3[m], sets[1][0])[1].T, sets[1][1].T)
        assert np.all(np.abs(vs3[m].reshape(4, 6)[:, 1] - stats[:, 1]) <= 1e-5 * split[1]), m
    for group in (2, 1):
        w, ts, vs = run(group)
        assert np.array_equal(w.view(np.uint32), w3.view(np.uint32)) and np.array_equal(ts, ts3)
        assert np.array_equal(vs.view(np.uint64), vs3.view(np.uint64)), group
