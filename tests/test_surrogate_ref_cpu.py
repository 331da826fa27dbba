"""The yardsticks of tests/surrogate_ref.py checked on the CPU: the per-sample gradient terms against torch fp64 autograd, the error sums
against the notebook's three numpy expressions, and the preconditions of every case the GPU tests list (tests/test_gpu_surrogate_trainer.py,
the gradient tests of tests/test_gpu_surrogate_train.py and tests/test_gpu_surrogate_stencil.py)."""
import json
import os

import numpy as np
import pytest

import surrogate_ref as sr


@pytest.mark.parametrize("n_in", [5, 9])
@pytest.mark.parametrize("batch", [1, 3, 65, 300])
def test_grad_terms_match_torch_fp64_autograd(n_in, batch):
    import torch
    w, x, y = sr.gradient_case(n_in, batch)
    terms = sr.grad_terms(n_in, w, x.T, y.T)
    assert terms.shape == (batch, sr.n_par(n_in)) and terms.dtype == np.float64
    g, T, loss, mae = sr.grad_summary(terms)
    P = sr.torch_model(w)
    out = sr.torch_forward(P, torch.tensor(x.T.astype(np.float64)))
    ref = torch.nn.functional.mse_loss(out, torch.tensor(y.T.astype(np.float64)))
    ref.backward()
    g_ref = np.concatenate([p.grad.numpy().ravel() for p in P])
    assert np.max(np.abs(g - g_ref)) <= 1e-12 * np.max(np.abs(g_ref))
    assert abs(loss - float(ref.detach())) <= 1e-12 * float(ref.detach())
    assert abs(mae - float((out.detach() - torch.tensor(y.T.astype(np.float64))).abs().mean())) <= 1e-12 * mae
    assert np.all(T >= np.abs(g)) and np.all(T > 0)
    assert sr.rho(g_ref, g, T) < 1e-3                                 # fp64 against fp64, in units of an fp32 rounding


def test_fp32_evaluations_are_fp32_and_differ():
    """The two fp32 evaluations are what they say: fp32 close to the fp64 gradient, not the fp64 gradient itself, and not each other."""
    w, x, y = sr.gradient_case(5, 1024)
    g_ref, T, loss, _ = sr.grad_summary(sr.grad_terms(5, w, x.T, y.T))
    ga, la = sr.grad_fp32_torch(5, w, x.T, y.T)
    gb = sr.grad_fp32_index_order(5, w, x.T, y.T)
    for g in (ga, gb):
        assert np.array_equal(g, g.astype(np.float32).astype(np.float64))
        assert 0.05 < sr.rho(g, g_ref, T) < 1e3
        assert np.max(np.abs(g - g_ref)) <= 1e-5 * np.max(np.abs(g_ref))
    assert not np.array_equal(ga, gb)
    assert abs(la - loss) <= 1e-6 * loss


def notebook_metrics(output_test, predict_test):
    """The training notebook's test cell (tests/golden/surrogate_notebook_metrics.json quotes its first expression), sample-major arrays."""
    return {"max_relative_error": np.amax(np.abs(output_test - predict_test), axis=0) / np.amax(np.abs(output_test), axis=0),
            "mean_relative_error": np.mean(np.abs(output_test - predict_test), axis=0) / np.mean(np.abs(output_test), axis=0),
            "mean_relative_bias": np.mean(output_test - predict_test, axis=0) / np.mean(np.abs(output_test), axis=0)}


@pytest.mark.parametrize("n", [1, 2, 257, 40001])
def test_error_sums_ref_matches_the_notebook_expressions(n):
    golden = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "surrogate_notebook_metrics.json")))
    assert "np.amax(np.abs(output_test - predict_test), axis=0) / np.amax(np.abs(output_test), axis=0)" in golden["definition"]
    from miniweatherml_amd.surrogate_train import _metrics
    pred, y = sr.errors_case(n, 2)
    for s in range(2):
        stats, mass = sr.error_sums_ref(pred[s], y)
        want = notebook_metrics(y.T.astype(np.float64), pred[s].T.astype(np.float64))
        got, product = sr.metrics_of(stats, n), _metrics(stats)
        for key in want:
            assert np.allclose(got[key], want[key], rtol=1e-12, atol=0), key
            assert np.array_equal(got[key], np.asarray(product[key])), key          # the product's own arithmetic on the same sums
        d = y.astype(np.float64) - pred[s].astype(np.float64)
        assert abs(got["test_loss"] - np.mean(d * d)) <= 1e-12 * np.mean(d * d)
        assert np.array_equal(stats[:, 4], np.max(np.abs(d), axis=1)) and np.array_equal(stats[:, 5], np.max(np.abs(y), axis=1))
        assert np.all(mass >= np.abs(stats[:, :4])) and np.array_equal(mass[:, 2], stats[:, 1])
        assert np.all(stats[0, 3] > 0) and np.all(y[0] < 0)                    # the all-negative column
        assert np.argmax(np.abs(y[1])) == n - 1 and np.argmax(np.abs(d[1])) == n - 1   # the outlier at the last index
        assert n < 257 or abs(stats[2, 2]) < 0.5 * stats[2, 1]                                   # signed differences: sum d is not sum |d|
    assert not np.array_equal(sr.error_sums_ref(pred[0], y)[0], sr.error_sums_ref(pred[1], y)[0])


def test_error_cases_tell_the_sets_apart():
    for n in sr.ERROR_SIZES[:6]:
        pred, y = sr.errors_case(n, 5)
        stats = [sr.error_sums_ref(pred[s], y)[0] for s in range(5)]
        for a in range(5):
            for b in range(a):
                assert np.all(stats[a][:, :3] != stats[b][:, :3]) and stats[a][1, 4] != stats[b][1, 4], (n, a, b)


@pytest.mark.parametrize("n_in", [5, 9])
def test_gradient_cases_meet_their_preconditions(n_in):
    for batch in sr.GRAD_BATCHES:
        w, x, y = sr.gradient_case(n_in, batch)
        assert x.shape == (n_in, batch) and y.shape == (4, batch) and w.dtype == x.dtype == y.dtype == np.float32
        assert sr.signs_ok(n_in, w, x), batch
        g_ref, T, _, _ = sr.grad_summary(sr.grad_terms(n_in, w, x.T, y.T))
        assert np.all(g_ref != 0.0) and np.all(T > 0), batch                  # every entry is exercised
        if batch <= 1024:
            cpu = sr.fp32_rho(n_in, w, x.T, y.T, g_ref, T)
            assert 0.25 <= cpu <= 100, (batch, cpu)                            # the right-hand side of the rho assertion is a usable number


@pytest.mark.parametrize("n_in", [5, 9])
def test_near_fit_cases_cancel(n_in):
    """At least half the entries add up 10 times more than what is left: T_e / |g_e| >= 10."""
    for batch in sr.NEAR_FIT_BATCHES:
        w, x, y = sr.near_fit_case(n_in, batch)
        assert sr.signs_ok(n_in, w, x)
        g_ref, T, loss, _ = sr.grad_summary(sr.grad_terms(n_in, w, x.T, y.T))
        share = float(np.mean(T >= 10 * np.abs(g_ref)))
        assert share >= 0.5, (batch, share)
        assert 0.5e-4 < loss < 2e-4                                            # mean r^2 of 1e-2 N(0, 1)


def test_prepare_cases_keep_every_set_non_empty():
    from miniweatherml_amd import surrogate_train as st
    cases = sr.prepare_cases()
    assert {c[0] for c in cases if c[1:] == sr.SPLITS[0]} == set(sr.PREPARE_SIZES)
    assert {c[0] for c in cases if c[1:] == sr.SPLITS[1]} == set(sr.PREPARE_SIZES) - {3}
    for n, ts, vs in cases:
        assert min(st.split_sizes(n, ts, vs)) >= 1 and sum(st.split_sizes(n, ts, vs)) == n
        assert n < 2 ** 24                                                     # the permutation case stores the index in fp32
    assert max(sr.PREPARE_SIZES) > 4096 * 256                                 # beyond one pass of the kernel's grid
    for n in (5, 257):
        x, y = sr.raw_samples(n, 9, n)
        sets = sr.host_sets(x, y, 3)
        assert [len(s[0]) for s in sets] == list(st.split_sizes(n)) and sets[0][0].dtype == np.float32
        allx = np.concatenate([s[0] for s in sets])
        assert allx.min() == 0.0 and allx.max() == 1.0 and np.all(allx.min(0) == 0.0) and np.all(allx.max(0) == 1.0)


def test_edge_configurations_have_the_shapes_they_are_there_for():
    from miniweatherml_amd import surrogate_train as st
    for c in sr.CONFIGS.values():
        assert st.split_sizes(c["n"]) == c["split"] and -(-c["split"][0] // c["batch"]) == c["steps"]
    a, b, c, d, e = [sr.CONFIGS[k] for k in "abcde"]
    assert a["batch"] == 1 and b["split"][0] < b["batch"] and c["batch"] == st.MAX_BATCH and c["split"][0] % c["batch"] == 4608
    assert d["split"][0] % d["batch"] == 0 and e["split"][0] % e["batch"] != 0 and e["lr"] == 1e-2


def test_replay_in_fp32_stays_near_the_fp64_replay():
    """The replay function in both precisions on a small run: same batch order, so the deviation is fp32 rounding alone."""
    import torch
    x, y = sr.raw_samples(2000, 5, 1)
    sets = sr.host_sets(x, y, 5)
    w64, h64 = sr.replay(torch.float64, sets, 5, 100, 2)
    w32, h32 = sr.replay(torch.float32, sets, 5, 100, 2)
    dev = sr.deviations(w32, h32, w64, h64)
    assert 0 < dev[0] <= 1e-5 and max(dev[1:]) <= 1e-5, dev
    assert len(h64["loss"]) == 2 and h64["loss"][1] < h64["loss"][0]
    from miniweatherml_amd import surrogate_train as st
    assert np.max(np.abs(w64 - st.initial_weights(5, 1)[0])) > 1e-3


def test_bias_correction_matches_the_kernels_fp32_beta2():
    """The kernel's second-moment recursion runs with fp32(0.999); its bias correction has to be built from the same number
    (surrogate_train.kernel_nadam_table).  Emulated on the CPU with exact gradients, 64 steps: with the matching table the weights stay
    within fp32 rounding of the fp64 replay, with 1 - 0.999^t every step is 6.4e-6 too long and the deviation is an order of magnitude
    larger (measured here: 3.1e-7 against 4.9e-6 of max|w|; torch's own fp32 replay reaches 1e-6 on such runs, hence the bound)."""
    import torch
    from miniweatherml_amd import surrogate_train as st
    x, y = sr.raw_samples(4000, 5, 2)
    sets = sr.host_sets(x, y, 5)
    w64, _ = sr.replay(torch.float64, sets, 5, 80, 2)
    steps = 2 * 32
    dev = lambda tab: float(np.max(np.abs(sr.emulate_trainer(sets, 5, 80, 2, tab) - w64)) / np.max(np.abs(w64)))          # noqa: E731
    good, biased = dev(st.kernel_nadam_table(steps)), dev(st.nadam_table(steps))
    print("matching table %.2e, 1 - 0.999^t %.2e" % (good, biased))
    assert good <= 1e-6
    assert biased >= 5 * good
    b = np.float32(st.NADAM["beta2"])
    assert np.float32(1) - b == np.float32(1.0 - float(b)) and abs((1.0 - float(b)) / 1e-3 - 1.0) > 1.2e-5        # 1 - b is exact, and not 1e-3
    tab = st.kernel_nadam_table(5)
    assert np.array_equal(tab[:, 2], (1.0 - float(b) ** np.arange(1, 6)).astype(np.float32))
    assert np.array_equal(tab[:, :2], st.nadam_table(5)[:, :2])
