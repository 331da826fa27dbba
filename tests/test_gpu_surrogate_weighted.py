"""Weighted surrogate training on the MI355X: mw_surrogate_prepare_column bit for bit, the weighted batch gradient
in its exact relations to the unweighted one and against the fp64 weighted reference, one weighted epoch bit for bit at w = 1, the
independence of the models, the trajectory against the weighted fp64 replay, the weighted error sums, and train_surrogate end to end with
file weights and per-file metrics.  The reference is tests/weighted_ref.py (checked on the CPU by tests/test_surrogate_weighted_cpu.py).

Trajectory deviations against the weighted torch fp64 replay (weighted_ref.replay), sample weights log-uniform in [2^-4, 2^4]; `fp32 replay`
= the same replay in torch fp32 on the CPU against the fp64 one, which is the yardstick: the kernel's weights may deviate 4 times as far,
each of its series 10 times as far (floor 4 x 2^-24 = 2.4e-7).  Columns: max|dw| / max|w|, then the largest relative deviation of loss,
mean_absolute_error, val_loss, val_mean_absolute_error over the epochs.  MEASURED on the MI355X:

configuration             max|dw|  loss     mae      val_loss val_mae
(a) single   kernel      6.66e-07 4.24e-08 2.60e-08 4.93e-08 1.30e-08
             fp32 replay 1.24e-06 8.43e-08 4.44e-08 2.55e-07 6.51e-08
             ratio       0.54     0.50     0.59     0.19     0.20
(d) single   kernel      3.64e-07 3.77e-08 1.37e-08 8.55e-08 4.45e-08
             fp32 replay 3.56e-07 3.27e-08 7.82e-09 6.74e-08 5.04e-09
             ratio       1.02     1.15     1.75     1.27     8.83
(e) single   kernel      3.46e-07 3.82e-08 1.69e-08 1.55e-07 8.82e-08
             fp32 replay 6.03e-07 2.22e-07 1.26e-07 7.73e-07 2.34e-07
             ratio       0.57     0.17     0.13     0.20     0.38
(a) stencil  kernel      9.15e-07 5.25e-08 2.31e-08 1.33e-08 4.19e-09
             fp32 replay 1.18e-06 6.99e-08 3.26e-08 3.18e-08 2.03e-08
             ratio       0.78     0.75     0.71     0.42     0.21
(d) stencil  kernel      3.68e-07 5.90e-08 2.85e-08 1.41e-07 7.16e-08
             fp32 replay 4.06e-07 8.09e-08 4.05e-08 1.78e-07 1.62e-07
             ratio       0.91     0.73     0.70     0.79     0.44

The largest ratio is 8.83 (validation MAE of (d) single, where the fp32 replay happens to land 5e-9 from the fp64 one; the floor of 2.4e-7
decides that limit); no kernel deviation is above 9.2e-7 for the weights or 1.6e-7 for a series.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import surrogate_ref as sr
import weighted_ref as wr
from test_surrogate_train_cpu import write_sample_file

pytestmark = pytest.mark.gpu

FLOOR = 4 * sr.U32
TINY32 = float(np.finfo(np.float32).tiny)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. mw_surrogate_prepare_column
def device_column(col, seed, n_train, n_val):
    import torch
    from miniweatherml_amd import capi
    n = len(col)
    src = torch.from_numpy(np.ascontiguousarray(col, np.float32)).cuda()
    outs = [torch.full((k,), float("nan"), dtype=torch.float32, device="cuda") for k in (n_train, n_val, n - n_train - n_val)]
    capi.check(capi.lib().mw_surrogate_prepare_column(n, ptr(src), seed, n_train, n_val, *[ptr(t) for t in outs], None))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 1])
@pytest.mark.parametrize("n", [3, 17, 256, 257, 65537, 4096 * 256 + 777])
def test_column_prepare_is_bitwise_the_preshuffle(mw, n, seed):
    """The column holds arange (distinct values, exact in fp32 below 2^24): a wrong index cannot hide.  The last n is above one full
    stride of the capped grid (4096 blocks x 256 threads).  Every split of surrogate_ref.SPLITS that leaves no set empty."""
    from miniweatherml_amd import surrogate_train as st
    col = np.arange(n, dtype=np.float32)
    ran = 0
    for ts, vs in sr.SPLITS:
        n_train, n_val, n_test = st.split_sizes(n, ts, vs)
        if min(n_train, n_val, n_test) < 1:
            continue
        got, want = device_column(col, seed, n_train, n_val), wr.split_column(col, seed, n_train, n_val)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (n, ts, vs, int(np.sum(bits(g) != bits(w))))
        ran += 1
    assert ran >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the weighted batch gradient: exact relations
@pytest.mark.parametrize("n_in", [5, 9])
@pytest.mark.parametrize("batch", [1, 3, 64, 65, 256, 257, 300])
def test_gradient_exact_relations(mw, n_in, batch):
    """w = 1: the bits of mw_surrogate_batch_grad_v2.  w = 2^-3 and w = 2^4: v2's gradient and loss times that power of two, bit for bit --
    scaling the D row by a power of two scales every product, every partial sum and the result exactly while nothing leaves the normal
    range; the compared values are asserted to be normal."""
    w, x, y = sr.gradient_case(n_in, batch)
    g0, l0 = wr.device_batch_grad_v2(n_in, w, x, y)
    assert np.all(np.isfinite(g0)) and np.isfinite(l0)
    for scale in (1.0, 2.0 ** -3, 2.0 ** 4):
        g, loss = wr.device_batch_grad_w(n_in, w, x, y, np.full(batch, scale, np.float32))
        want_g, want_l = g0 * np.float32(scale), l0 * np.float32(scale)
        for v in (g, want_g, g0, np.array([loss, want_l, l0])):
            assert np.all((np.abs(v) >= TINY32) | (v == 0)), "a subnormal among the compared values"
        assert np.array_equal(bits(g), bits(want_g)), (scale, int(np.sum(bits(g) != bits(want_g))))
        assert bits(np.array([loss]))[0] == bits(np.array([want_l]))[0], (scale, loss, want_l)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the weighted batch gradient: general weights
@pytest.mark.parametrize("n_in", [5, 9])
@pytest.mark.parametrize("batch", [1, 64, 65, 255, 256, 257, 300, 1024, 8192])
def test_gradient_general_weights(mw, n_in, batch):
    """Log-uniform weights in [2^-4, 2^4], and a second vector of ones with 16s and zeros planted at positions 0, 63, 64, 255, 256 and
    B - 1: rho(kernel) <= 4 rho(fp32 on the CPU), both against the fp64 weighted terms; the loss against the fp64 one."""
    w, x, y = sr.gradient_case(n_in, batch)
    for name, wt in (("log-uniform", wr.log_uniform_weights(batch, 1)), ("planted", wr.planted_weights(batch))):
        g, loss = wr.device_batch_grad_w(n_in, w, x, y, wt)
        wr.check_rho(n_in, w, x, y, wt, g.astype(np.float64), "%s, n_in %d, batch %d" % (name, n_in, batch))
        loss_ref = wr.weighted_summary(n_in, w, x.T, y.T, wt)[2]
        assert abs(float(loss) - loss_ref) <= 1e-6 * loss_ref, (name, abs(float(loss) - loss_ref) / loss_ref)


@pytest.mark.parametrize("n_in", [5, 9])
def test_gradient_general_weights_near_a_fit(mw, n_in):
    w, x, y = sr.near_fit_case(n_in, 300)
    wt = wr.log_uniform_weights(300, 2)
    g, _ = wr.device_batch_grad_w(n_in, w, x, y, wt)
    wr.check_rho(n_in, w, x, y, wt, g.astype(np.float64), "near fit, n_in %d" % n_in)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the weighted epoch
def device_epochs(n_in, K, x, y, wt, batch, epochs, seed):
    """`epochs` epochs of K models from the seeded initial weights on x (n_in, n), y (4, n); wt (n,) runs mw_surrogate_train_epoch_w, wt
    None mw_surrogate_train_epoch_v2.  Returns per epoch (params, m1, m2, stats)."""
    import torch
    from miniweatherml_amd import capi, surrogate_train as st
    n = x.shape[1]
    steps = (n + batch - 1) // batch
    L = capi.lib()
    dx, dy = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()
    dw = None if wt is None else torch.from_numpy(np.ascontiguousarray(wt, np.float32)).cuda()
    params = torch.from_numpy(st.initial_weights(seed, K, stencil=n_in == 9)).cuda()
    m1, m2 = torch.zeros_like(params), torch.zeros_like(params)
    table = torch.from_numpy(st.kernel_nadam_table(steps * epochs)).cuda()
    stats = torch.full((K, 2), float("nan"), dtype=torch.float64, device="cuda")
    out = []
    for e in range(epochs):
        tail = (n, batch, e, seed, ptr(params), ptr(m1), ptr(m2), ctypes.c_void_p(table.data_ptr() + e * steps * 12), 0.9, 0.999, 1e-7,
                ptr(stats), None)
        if wt is None:
            capi.check(L.mw_surrogate_train_epoch_v2(n_in, K, ptr(dx), ptr(dy), *tail))
        else:
            capi.check(L.mw_surrogate_train_epoch_w(n_in, K, ptr(dx), ptr(dy), ptr(dw), *tail))
        torch.cuda.synchronize()
        out.append(tuple(t.cpu().numpy().copy() for t in (params, m1, m2, stats)))
    return out


def epoch_case(n_in, n):
    rng = np.random.default_rng([n_in, n])
    return rng.random((n_in, n), dtype=np.float32), rng.random((4, n), dtype=np.float32)


@pytest.mark.parametrize("n_in", [5, 9])
def test_epoch_at_weight_one_is_the_unweighted_epoch_bit_for_bit(mw, n_in):
    """700 samples in batches of 300, 300, 100, three models, epochs 0 and 1: parameters, both moments and the sums of
    mw_surrogate_train_epoch_w at w = 1 are those of _v2.
    With w = 2^-1 the sums are _v2's times 2^-1 exactly WHERE THE WEIGHTS ARE THE SAME: Nadam is not scale-free in fp32 (the eps in its
    denominator), so from the second step on the two runs stand at different weights and their batches' sums differ in the last digits.
    The relation is therefore asserted on one-step epochs -- the 700 samples as one batch (three chunks, the last partial) and 300 samples
    at batch 300 -- and the three-step epoch's deviation is printed."""
    x, y = epoch_case(n_in, 700)
    ref = device_epochs(n_in, 3, x, y, None, 300, 2, 11)
    got = device_epochs(n_in, 3, x, y, np.ones(700, np.float32), 300, 2, 11)
    for e in range(2):
        for a, b, what in zip(got[e], ref[e], ("params", "m1", "m2", "stats")):
            assert np.all(np.isfinite(b)) and np.array_equal(a, b), (e, what)
    assert not np.array_equal(ref[0][0], ref[1][0])                        # (it trains)
    half = np.full(700, 0.5, np.float32)
    for n, batch in ((700, 1024), (300, 300)):
        r1 = device_epochs(n_in, 3, x[:, :n], y[:, :n], None, batch, 1, 11)[0]
        h1 = device_epochs(n_in, 3, x[:, :n], y[:, :n], half[:n], batch, 1, 11)[0]
        assert np.array_equal(h1[3], 0.5 * r1[3]) and np.all(r1[3] > 0), (n, batch)
    h3 = device_epochs(n_in, 3, x, y, half, 300, 1, 11)[0]
    print("three steps at w = 1/2: max relative deviation of the sums from half the unweighted ones %.2e" % np.max(np.abs(h3[3] / (0.5 * ref[0][3]) - 1)))


@pytest.mark.parametrize("n_in", [5, 9])
def test_weighted_models_are_independent(mw, n_in):
    """Model 1 of a K = 3 weighted run is the K = 1 run with seed + 1, bit for bit."""
    x, y = epoch_case(n_in, 700)
    wt = wr.log_uniform_weights(700, 3)
    three = device_epochs(n_in, 3, x, y, wt, 300, 2, 20)
    one = device_epochs(n_in, 1, x, y, wt, 300, 2, 21)
    for e in range(2):
        for a, b, what in zip(three[e], one[e], ("params", "m1", "m2", "stats")):
            assert np.array_equal(a[1], b[0]), (e, what)
    assert not np.array_equal(three[1][0][0], three[1][0][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the trajectory
@pytest.mark.parametrize("name,stencil", [("a", False), ("d", False), ("e", False), ("a", True), ("d", True)],
                         ids=lambda v: v if isinstance(v, str) else ("stencil" if v else "single"))
def test_trajectory_against_the_weighted_replay(mw, tmp_path, name, stencil):
    """(a) batch 1, 256 steps; (d) no partial batch; (e) learning rate 1e-2 at batch 257.  The yardstick is the torch fp32 replay's own
    deviation from the fp64 replay, never the kernel: weights within 4 times it (the project's gradient factor), each series within 10
    times it (section 13's "no ratio above 10 is left"), each limit at least 4 x 2^-24."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    from test_gpu_surrogate_trainer import configuration_samples
    c = sr.CONFIGS[name]
    ins, feats, outs = configuration_samples(name, stencil)
    wt = wr.log_uniform_weights(c["n"], 4)
    path = write_sample_file(tmp_path / "s.nc", [(ins, outs)])
    r = st.train_surrogate([path], epochs=c["epochs"], batch_size=c["batch"], learning_rate=c["lr"], seed=sr.CONFIG_SEED, stencil=stencil,
                           sample_weights=wt)
    assert (r["n_train"], r["n_val"], r["n_test"]) == c["split"] and r["weighted"] is True and r["file_weights"] is None
    sets = sr.host_sets(feats, outs, sr.CONFIG_SEED)
    wsets = wr.split_column(wt, sr.CONFIG_SEED, r["n_train"], r["n_val"])[:2]
    w64, h64 = wr.replay(torch.float64, sets, wsets, sr.CONFIG_SEED, c["batch"], c["epochs"], c["lr"], stencil)
    w32, h32 = wr.replay(torch.float32, sets, wsets, sr.CONFIG_SEED, c["batch"], c["epochs"], c["lr"], stencil)
    dev = sr.deviations(r["weights"][0], r["history"][0], w64, h64)
    yard = sr.deviations(w32, h32, w64, h64)
    tag = "(%s) %s" % (name, "stencil" if stencil else "single ")
    print("TRAJECTORY %s kernel      %s" % (tag, " ".join("%.2e" % v for v in dev)))
    print("TRAJECTORY %s fp32 replay %s" % (tag, " ".join("%.2e" % v for v in yard)))
    sr.check_test_metrics(r, sets[2], "(%s)" % name)                       # the test metrics stay unweighted
    limits = [max(4 * yard[0], FLOOR)] + [max(10 * v, FLOOR) for v in yard[1:]]
    assert all(d <= lim for d, lim in zip(dev, limits)), (dev, limits)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the weighted error sums
def check_sums(got, pred, y, wt, n):
    worst = 0.0
    for s in range(pred.shape[0]):
        stats, mass = wr.error_sums_ref(pred[s], y, wt)
        assert np.array_equal(got[s][:, 4:], stats[:, 4:]), (s, got[s][:, 4:], stats[:, 4:])
        err, bound = np.abs(got[s][:, :4] - stats[:, :4]), n * 2.0 ** -52 * mass
        assert np.all(err <= bound), (s, err, bound)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    return worst


@pytest.mark.parametrize("nsets", [1, 3])
@pytest.mark.parametrize("n", [1, 257, 128 * 256 + 1])
def test_weighted_error_sums(mw, n, nsets):
    """w = 1: the bits of mw_surrogate_errors.  General weights: every sum within n 2^-52 sum|terms| of the reference's, both maxima equal
    to the reference's over w > 0.  The set's largest |d| of every output planted on samples of weight zero: it is not the maximum
    returned.  Indicator weights of three interleaved groups: the three calls' sums add up to the unweighted call's, their maxima's
    maximum is the unweighted maximum."""
    pred, y = sr.errors_case(n, nsets)
    k = n // 2
    pred[:, (0, 2, 3), k] = y[(0, 2, 3), k] + np.float32(50.0)            # with errors_case's own outlier of output 1 at n - 1
    plain = wr.device_errors(pred, y)
    assert np.array_equal(wr.device_errors(pred, y, np.ones(n, np.float32)), plain)
    assert np.all(plain[:, (0, 2, 3), 4] >= 49.0) and np.all(plain[:, 1, 4] >= 1500.0)
    wt = wr.log_uniform_weights(n, 5)
    worst = check_sums(wr.device_errors(pred, y, wt), pred, y, wt, n)
    assert np.array_equal(wr.device_errors(pred, y, wt)[:, :, 4:], plain[:, :, 4:])           # all weights positive: the maxima of all samples
    wz = wt.copy()
    wz[[k, n - 1]] = 0.0
    got = wr.device_errors(pred, y, wz)
    worst = max(worst, check_sums(got, pred, y, wz, n))
    assert np.all(got[:, :, 4] < 10.0) and np.all(got[:, 1, 5] < 1000.0), "a sample of weight zero set a maximum"
    if n == 1:
        assert np.all(got == 0.0)                                          # no sample exists for the call
    parts = [wr.device_errors(pred, y, (np.arange(n) % 3 == g).astype(np.float32)) for g in range(3)]
    for s in range(nsets):
        _, mass = sr.error_sums_ref(pred[s], y)
        assert np.all(np.abs(sum(p[s][:, :4] for p in parts) - plain[s][:, :4]) <= n * 2.0 ** -52 * mass), s
        assert np.array_equal(np.max([p[s][:, 4:] for p in parts], axis=0), plain[s][:, 4:]), s
        for g in range(3):
            check_sums(parts[g][s:s + 1], pred[s:s + 1], y, (np.arange(n) % 3 == g).astype(np.float32), n)
    print("n %d, %d sets: worst |sum - reference| / (n 2^-52 sum|terms|) = %.2e" % (n, nsets, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. end to end
RUN = dict(epochs=wr.E2E["epochs"], batch_size=wr.E2E["batch"], models=wr.E2E["models"], seed=wr.E2E["seed"])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("weighted")
    return [write_sample_file(d / name, [chunk]) for name, chunk in zip(("a.nc", "b.nc"), wr.two_files())]


@pytest.fixture(scope="module")
def plain_run(mw, files, tmp_path_factory):
    """The run without the new arguments, written to a directory (the direction test continues it)."""
    from miniweatherml_amd import surrogate_train as st
    out = str(tmp_path_factory.mktemp("plain"))
    return st.train_surrogate(files, out, **RUN), out


def test_file_weights_of_one_change_nothing_but_the_new_keys(mw, files, plain_run, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    r0, out0 = plain_run
    assert "weighted" not in r0 and "file_weights" not in r0 and "group_metrics" not in r0
    r1 = st.train_surrogate(files, str(tmp_path / "w"), file_weights=(1, 1), **RUN)
    assert open(os.path.join(out0, "weights.txt"), "rb").read() == open(tmp_path / "w" / "weights.txt", "rb").read()
    assert np.array_equal(r0["weights"], r1["weights"]) and r0["best_model"] == r1["best_model"] and r0["history"] == r1["history"]
    assert r0["test_metrics"] == r1["test_metrics"]
    j0, j1 = json.load(open(os.path.join(out0, "history.json"))), json.load(open(tmp_path / "w" / "history.json"))
    assert set(j1) - set(j0) == {"weighted", "file_weights"} and set(j0) <= set(j1)
    assert j1["weighted"] is True and j1["file_weights"] == [1.0, 1.0]
    for key in j0:
        if key != "epoch_seconds":                                         # (wall-clock times)
            assert j0[key] == j1[key], key
    assert sorted(os.listdir(out0)) == sorted(os.listdir(tmp_path / "w"))


def group_reference(r, g, which):
    """(samples, labels) of file g in the set `which` (1 = validation, 2 = test) as the host restates the prepare step."""
    feats, outs, gi = wr.two_file_arrays()
    sets = sr.host_sets(feats, outs, r["split_seed"])
    gsets = wr.split_column(gi, r["split_seed"], r["n_train"], r["n_val"])
    pick = gsets[which] == g
    return sets[which][0][pick], sets[which][1][pick], [int((gs == g).sum()) for gs in gsets]


def test_group_metrics_with_file_weights(mw, files, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    r = st.train_surrogate(files, str(tmp_path / "o"), file_weights=(1, 8), group_metrics=True, **RUN)
    js = json.load(open(tmp_path / "o" / "history.json"))
    assert r["weighted"] is True and r["file_weights"] == [1.0, 8.0] and js["file_weights"] == [1.0, 8.0]
    gm = r["group_metrics"]
    assert js["group_metrics"] == gm and [g["file"] for g in gm] == files and [g["weight"] for g in gm] == [1.0, 8.0]
    keys = {"file", "weight", "n_train", "n_val", "n_test", "val_loss", "val_mean_absolute_error", "test_loss", "max_relative_error",
            "mean_relative_error", "mean_relative_bias"}
    assert all(set(g) == keys for g in gm)
    for k in ("n_train", "n_val", "n_test"):
        assert sum(g[k] for g in gm) == r[k] and all(g[k] > 0 for g in gm)
    assert [g["n_train"] + g["n_val"] + g["n_test"] for g in gm] == [wr.N_A, wr.N_B]
    # the files' test sums add up to the whole test set's: two fp64 sums of non-negative terms, each within n 2^-52 of its exact value
    lhs, rhs = sum(g["n_test"] * g["test_loss"] for g in gm), r["n_test"] * r["test_metrics"]["test_loss"]
    assert abs(lhs - rhs) <= (2 * r["n_test"] + 8) * 2.0 ** -52 * rhs, (lhs, rhs)
    best = r["weights"][r["best_model"]]
    for g, rec in enumerate(gm):
        sx, sy, counts = group_reference(r, g, 2)
        assert counts == [rec["n_train"], rec["n_val"], rec["n_test"]]
        fake = {"n_test": rec["n_test"], "weights": r["weights"], "best_model": r["best_model"],
                "test_metrics": {k: rec[k] for k in ("max_relative_error", "mean_relative_error", "mean_relative_bias", "test_loss")}}
        sr.check_test_metrics(fake, (sx, sy), "file %d" % g)
        vx, vy, _ = group_reference(r, g, 1)
        d = sr.forward64(best, vx)[1] - vy.astype(np.float64)
        mean_d = np.abs(d).mean()                                          # check_test_metrics' tolerances: the MFMA forward is held to 1e-5
        assert abs(rec["val_loss"] - np.mean(d * d)) <= 2e-5 * mean_d + 1e-10
        assert abs(rec["val_mean_absolute_error"] - mean_d) <= 1e-5


def test_a_file_of_weight_zero_is_an_evaluation_group(mw, files):
    from miniweatherml_amd import surrogate_train as st
    r = st.train_surrogate(files, file_weights=(1, 0), group_metrics=True, **RUN)
    b = r["group_metrics"][1]
    assert b["weight"] == 0.0 and b["n_train"] > 0 and b["test_loss"] is not None and np.isfinite(b["test_loss"]) and b["test_loss"] > 0
    sw = np.repeat(np.float32([1.0, 0.0]), [wr.N_A, wr.N_B])
    r2 = st.train_surrogate(files, sample_weights=sw, group_metrics=True, **RUN)
    assert np.array_equal(r["weights"], r2["weights"]) and r["history"] == r2["history"]
    assert r2["file_weights"] is None and r2["group_metrics"][1]["weight"] is None
    assert r2["group_metrics"][1]["test_loss"] == b["test_loss"]
    r1 = st.train_surrogate(files, file_weights=(1, 1), **RUN)
    assert not np.array_equal(r["weights"], r1["weights"])                 # (the zero took file B out of the fit)
    with pytest.raises(st.SurrogateTrainError, match="positive weight"):
        st.train_surrogate(files, file_weights=(0, 0), group_metrics=True, **RUN)


def test_group_metrics_without_weights_and_an_empty_group(mw, files, tmp_path):
    """group_metrics alone leaves the fit as it is (no `weighted` key); a file without a sample in a set reports None there."""
    from miniweatherml_amd import surrogate_train as st
    r = st.train_surrogate(files, group_metrics=True, **RUN)
    assert "weighted" not in r and [g["weight"] for g in r["group_metrics"]] == [1.0, 1.0]
    rng = np.random.default_rng(6)
    one = write_sample_file(tmp_path / "one.nc", [(rng.random((1, 5, 2), dtype=np.float32), rng.random((1, 4), dtype=np.float32))])
    empty = write_sample_file(tmp_path / "empty.nc", [])
    r = st.train_surrogate(files + [one, empty], group_metrics=True, **RUN)
    assert len(r["group_metrics"]) == 4                                    # a last file without samples is a group too
    g = r["group_metrics"][3]
    assert (g["n_train"], g["n_val"], g["n_test"]) == (0, 0, 0) and g["val_loss"] is None and g["test_loss"] is None
    g = r["group_metrics"][2]
    assert g["n_train"] + g["n_val"] + g["n_test"] == 1
    for k, keys in (("n_val", ("val_loss", "val_mean_absolute_error")), ("n_test", ("test_loss", "max_relative_error", "mean_relative_bias"))):
        assert all((g[key] is None) == (g[k] == 0) for key in keys), g
    json.dumps(r["group_metrics"])


def test_direction_a_heavier_file_is_fitted_better(mw, files, plain_run):
    """The model of the run without weights, continued (--init) at learning rate 1e-3 with file weights (1, 16), ends at a lower
    unweighted test loss on file B than continued with (1, 1).  The ordering holds in the weighted fp64 replay by a factor 6.6
    (tests/test_surrogate_weighted_cpu.py); the ordering is what is asserted here."""
    from miniweatherml_amd import surrogate_train as st
    _, out0 = plain_run
    kw = dict(epochs=wr.CONTINUE["epochs"], batch_size=wr.E2E["batch"], models=1, seed=wr.E2E["seed"], learning_rate=wr.CONTINUE["lr"],
              init=out0, group_metrics=True)
    plain = st.train_surrogate(files, file_weights=(1, 1), **kw)["group_metrics"][1]["test_loss"]
    heavy = st.train_surrogate(files, file_weights=(1, wr.CONTINUE["heavy"]), **kw)["group_metrics"][1]["test_loss"]
    print("file B test loss after the continuation: weights (1, 1) %.4e, (1, 16) %.4e" % (plain, heavy))
    assert heavy < plain


@pytest.mark.parametrize("option", ["stencil", "tendency"])
def test_file_weights_with_the_other_forms(mw, files, tmp_path, option):
    from miniweatherml_amd import surrogate_train as st
    paths = files
    if option == "stencil":
        paths = [write_sample_file(tmp_path / name, [chunk]) for name, chunk in zip(("a9.nc", "b9.nc"), wr.two_files(stencil=True))]
    r = st.train_surrogate(paths, str(tmp_path / "o"), file_weights=(1, 8), group_metrics=True, stencil=option == "stencil",
                           form="tendency" if option == "tendency" else None, **RUN)
    assert r["weighted"] is True and r["weights"].shape == (2, 144 if option == "stencil" else 104) and np.all(np.isfinite(r["weights"]))
    assert r["form"] == ("tendency" if option == "tendency" else "state") and len(r["group_metrics"]) == 2
    assert all(os.path.getsize(p) > 0 for p in r["files_written"]) and os.path.exists(tmp_path / "o" / "history.json")
    h = r["history"][r["best_model"]]
    assert all(np.isfinite(h[k]).all() and len(h[k]) == 2 for k in sr.SERIES)


def test_cli_with_file_weights_and_group_metrics(mw, files, tmp_path, capsys):
    from miniweatherml_amd import surrogate_train as st
    rc = st.main(files + ["--out", str(tmp_path / "o"), "--epochs", "2", "--batch-size", "64", "--models", "2", "--seed", "5",
                          "--file-weights", "1,8", "--group-metrics"])
    text = capsys.readouterr().out
    assert rc == 0
    lines = [ln for ln in text.splitlines() if ln.startswith("file ")]
    assert len(lines) == 2 and "(weight 1)" in lines[0] and "(weight 8)" in lines[1] and files[1] in lines[1]
    assert text.index("Mean relative bias") < text.index(lines[0])        # after the notebook's three metrics
    js = json.load(open(tmp_path / "o" / "history.json"))
    assert js["file_weights"] == [1.0, 8.0] and len(js["group_metrics"]) == 2
