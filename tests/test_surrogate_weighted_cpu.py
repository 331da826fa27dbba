"""Weighted surrogate training without a GPU: the four new entry points' declarations and refusals (which come
before the device check), train_surrogate's host refusals, the CLI's --file-weights, and the invariants of the reference
tests/weighted_ref.py that the GPU tests lean on -- weights of 1 are the unweighted reference, a weight of 2 is the sample twice, the
weighted replay at w = 1 is surrogate_ref.replay, and the direction test's ordering holds in the fp64 replay by a factor."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import surrogate_ref as sr
import weighted_ref as wr
from test_surrogate_train_cpu import random_chunks, write_sample_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mw_surrogate_prepare_column": 9, "mw_surrogate_train_epoch_w": 18, "mw_surrogate_batch_grad_w": 9, "mw_surrogate_errors_weighted": 8}
SENTINEL = -77.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entries_are_declared_and_exported_with_the_bindings_argument_counts(mw):
    from miniweatherml_amd import capi
    L = capi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mw_cdna4.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(capi.SYMBOLS[name][1]), name
        assert capi.SYMBOLS[name][0] is C.c_int and hasattr(L, name)
    doc = open(os.path.join(ROOT, "include", "mw_cdna4.h")).read()
    assert "0 * NaN" in doc and "not the sum of the" in doc                # the header says what the kernels do not check, and the divisor


def _buffers():
    """Sentinel-filled host arrays standing in for the device outputs (a refusal returns before anything could touch them)."""
    return {k: np.full(n, SENTINEL, dt) for k, n, dt in (("a", 64, np.float32), ("b", 64, np.float32), ("c", 64, np.float32),
                                                         ("stats", 8, np.float64), ("out", 48, np.float64))}


def _refused(L, rc, text, bufs):
    err = L.mw_last_error()
    assert rc != 0 and text in err and b"no HIP device" not in err, (rc, err)
    for k, a in bufs.items():
        assert np.all(a == SENTINEL), k


def test_every_refusal_comes_before_the_device_check(mw):
    """Each entry with ONE bad argument at a time (the others valid): the message names the argument check, never the missing device, and
    the outputs keep their sentinel.  No call here has all arguments valid, so none can launch."""
    from miniweatherml_amd import capi
    L = capi.lib()
    bufs = _buffers()
    p = lambda k: C.c_void_p(bufs[k].ctypes.data)                          # noqa: E731
    src = np.zeros(64, np.float32)
    s = C.c_void_p(src.ctypes.data)
    # mw_surrogate_prepare_column(n, col, seed, n_train, n_val, train_c, val_c, test_c, stream)
    good = [10, s, 0, 6, 2, p("a"), p("b"), p("c"), None]
    for i in (1, 5, 6, 7):
        a = list(good); a[i] = None
        _refused(L, L.mw_surrogate_prepare_column(*a), b"surrogate_prepare_column: null argument", bufs)
    for n, n_train, n_val in ((2, 1, 1), (10, 0, 2), (10, 6, 0), (10, 6, 4), (10, 10, 0), (10, 8, 3)):
        a = list(good); a[0], a[3], a[4] = n, n_train, n_val
        _refused(L, L.mw_surrogate_prepare_column(*a), b"surrogate_prepare_column: every set needs at least one sample", bufs)
    # mw_surrogate_train_epoch_w(n_in, models, x, y, w, n, batch, epoch, seed, params, m1, m2, table, beta1, beta2, eps, stats, stream)
    good = [5, 1, s, s, s, 10, 4, 0, 0, p("a"), p("b"), p("c"), s, 0.9, 0.999, 1e-7, p("stats"), None]
    for n_in in (0, 4, 6, 10):
        a = list(good); a[0] = n_in
        _refused(L, L.mw_surrogate_train_epoch_w(*a), b"n_in must be 5 (single cell) or 9 (stencil)", bufs)
    for i in (2, 3, 9, 10, 11, 12, 16):
        a = list(good); a[i] = None
        _refused(L, L.mw_surrogate_train_epoch_w(*a), b"surrogate_train_epoch: null argument", bufs)
    a = list(good); a[4] = None
    _refused(L, L.mw_surrogate_train_epoch_w(*a), b"null weights (the unweighted epoch is mw_surrogate_train_epoch_v2)", bufs)
    for models in (0, -1, capi.MW_SURROGATE_MAX_MODELS + 1):
        a = list(good); a[1] = models
        _refused(L, L.mw_surrogate_train_epoch_w(*a), b"surrogate_train_epoch: models must be in [1, 256]", bufs)
    for batch in (0, -3, 8193):
        a = list(good); a[6] = batch
        _refused(L, L.mw_surrogate_train_epoch_w(*a), b"surrogate_train_epoch: batch must be in [1, 8192]", bufs)
    for n, epoch in ((0, 0), (-5, 0), (10, -1)):
        a = list(good); a[5], a[7] = n, epoch
        _refused(L, L.mw_surrogate_train_epoch_w(*a), b"n must be >= 1 and epoch >= 0", bufs)
    # mw_surrogate_batch_grad_w(n_in, params, x, y, w, batch, grad, loss, stream)
    good = [9, s, s, s, s, 4, p("a"), p("b"), None]
    for n_in in (0, 7):
        a = list(good); a[0] = n_in
        _refused(L, L.mw_surrogate_batch_grad_w(*a), b"n_in must be 5 (single cell) or 9 (stencil)", bufs)
    for i in (1, 2, 3, 6, 7):
        a = list(good); a[i] = None
        _refused(L, L.mw_surrogate_batch_grad_w(*a), b"surrogate_batch_grad: null argument", bufs)
    a = list(good); a[4] = None
    _refused(L, L.mw_surrogate_batch_grad_w(*a), b"null weights (the unweighted gradient is mw_surrogate_batch_grad_v2)", bufs)
    for batch in (0, 8193):
        a = list(good); a[5] = batch
        _refused(L, L.mw_surrogate_batch_grad_w(*a), b"surrogate_batch_grad: batch must be in [1, 8192]", bufs)
    # mw_surrogate_errors_weighted(n, nsets, pred, y, w, workspace, out, stream)
    good = [10, 1, s, s, s, p("a"), p("out"), None]
    for i in (2, 3, 4, 5, 6):
        a = list(good); a[i] = None
        _refused(L, L.mw_surrogate_errors_weighted(*a), b"surrogate_errors: null argument", bufs)
    for n, nsets in ((0, 1), (10, 0), (10, 65536)):
        a = list(good); a[0], a[1] = n, nsets
        _refused(L, L.mw_surrogate_errors_weighted(*a), b"n must be >= 1 and nsets in [1, 65535]", bufs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host refusals and the CLI
def test_train_surrogate_refuses_bad_weights_on_the_host(mw, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    E = st.SurrogateTrainError
    rng = np.random.default_rng(8)
    fa = write_sample_file(tmp_path / "a.nc", random_chunks(rng, [200]))
    fb = write_sample_file(tmp_path / "b.nc", random_chunks(rng, [40]))
    run = lambda **kw: st.train_surrogate([fa, fb], device="cpu", **kw)    # noqa: E731  (a refusal comes before the device is touched)
    for fw in ((1.0,), (1.0, 1.0, 1.0)):
        with pytest.raises(E, match=r"file_weights: %d weights for 2 sample files" % len(fw)):
            run(file_weights=fw)
    with pytest.raises(E, match=r"sample_weights: 239 weights for 240 samples"):
        run(sample_weights=np.ones(239))
    with pytest.raises(E, match="non-finite weight"):
        run(file_weights=(1.0, float("nan")))
    with pytest.raises(E, match="non-finite weight .first at index 17"):
        run(sample_weights=np.where(np.arange(240) == 17, np.inf, 1.0))
    with pytest.raises(E, match="negative weight -1.0 at index 1"):
        run(file_weights=(1.0, -1.0))
    with pytest.raises(E, match="give one of them"):
        run(file_weights=(1.0, 1.0), sample_weights=np.ones(240))
    with pytest.raises(E, match="has a positive weight"):
        run(file_weights=(0.0, 0.0))
    # all TRAINING weights zero, though one sample of the validation set and one of the test set count
    n_train, n_val, _ = st.split_sizes(240)
    perm = st.preshuffle_permutation(240, 3)
    w = np.zeros(240)
    w[perm[n_train]] = w[perm[-1]] = 1.0
    with pytest.raises(E, match="no sample of the training set .153 of 240 samples, split seed 3."):
        run(sample_weights=w, seed=3)
    with pytest.raises(E, match="split seed 9"):
        run(sample_weights=np.where(np.arange(240) == st.preshuffle_permutation(240, 9)[n_train], 1.0, 0.0), seed=3, split_seed=9)
    w[perm[0]] = 1e-30                                                       # one positive training weight: the weights pass, the device is next
    assert st.check_training_weights(st.check_weights(240, np.zeros(240, int), 1, None, w), n_train, 3) is None


def test_read_samples_keeps_what_it_returned_and_adds_the_file_index(mw, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(2)
    files = [write_sample_file(tmp_path / ("%d.nc" % k), random_chunks(rng, sizes)) for k, sizes in enumerate(([5, 3], [4], [1, 1, 1]))]
    inputs, outputs, meta = st.read_samples(files)
    assert inputs.shape == (15, 5) and outputs.shape == (15, 4) and meta["files"] == files and meta["time_step_size"] == 0.5
    assert meta["file_counts"] == [8, 4, 3] and np.array_equal(meta["file_index"], np.repeat([0, 1, 2], [8, 4, 3]))
    w = st.check_weights(15, meta["file_index"], 3, file_weights=(1, 0, 25))
    assert w.dtype == np.float32 and np.array_equal(w, np.repeat([1.0, 0.0, 25.0], [8, 4, 3]))
    assert st.check_weights(15, meta["file_index"], 3) is None


def test_cli_parses_file_weights(mw, tmp_path, capsys):
    from miniweatherml_amd import surrogate_train as st
    assert st.parse_file_weights("1,1,25") == (1.0, 1.0, 25.0) and st.parse_file_weights("0.5") == (0.5,)
    assert st.parse_file_weights(" 2 , 1e-3") == (2.0, 1e-3)
    for bad in ("1;2", "a,b", "1,,2", ""):
        with pytest.raises(st.SurrogateTrainError, match="--file-weights"):
            st.parse_file_weights(bad)
    rng = np.random.default_rng(3)
    f = write_sample_file(tmp_path / "a.nc", random_chunks(rng, [100]))
    # the refusals reach the user as the CLI's exit status 2, before any device work
    for flag, msg in (("1,2", "2 weights for 1 sample files"), ("-1", "negative weight"), ("x", "--file-weights"), ("0", "positive weight")):
        assert st.main([f, "--out", str(tmp_path / "o"), "--device", "cpu", "--file-weights", flag, "--group-metrics"]) == 2
        assert msg in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's own invariants
@pytest.mark.parametrize("n_in", [5, 9])
def test_weights_of_one_are_the_unweighted_reference(n_in):
    w, x, y = sr.gradient_case(n_in, 300)
    one = np.ones(300, np.float32)
    assert np.array_equal(wr.weighted_terms(n_in, w, x.T, y.T, one), sr.grad_terms(n_in, w, x.T, y.T))
    a, b = wr.weighted_summary(n_in, w, x.T, y.T, one), sr.grad_summary(sr.grad_terms(n_in, w, x.T, y.T))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(wr.grad_fp32_index_order(n_in, w, x.T, y.T, one), sr.grad_fp32_index_order(n_in, w, x.T, y.T))
    ga, la = wr.grad_fp32_torch(n_in, w, x.T, y.T, one)
    gb, lb = sr.grad_fp32_torch(n_in, w, x.T, y.T)
    assert np.max(np.abs(ga - gb)) <= 4 * sr.U32 * np.max(np.abs(gb)) and abs(la - lb) <= 4 * sr.U32 * lb     # (mse_loss sums in another order)
    pred, t = sr.errors_case(257, 2)
    for s in range(2):
        sa, ma = wr.error_sums_ref(pred[s], t, np.ones(257, np.float32))
        sb, mb = sr.error_sums_ref(pred[s], t)
        assert np.array_equal(sa, sb) and np.array_equal(ma, mb)


def test_a_weight_of_two_is_the_sample_twice():
    """Exact arithmetic (math.fsum of the fp64 terms): doubling a term is exact, so the sums agree to the last bit."""
    n_in, B, k = 5, 65, 64
    w, x, y = sr.gradient_case(n_in, B)
    wt = np.ones(B)
    wt[k] = 2.0
    twice = lambda a: np.concatenate([a, a[:, k:k + 1]], axis=1)           # noqa: E731
    tw, td = wr.weighted_terms(n_in, w, x.T, y.T, wt), sr.grad_terms(n_in, w, twice(x).T, twice(y).T)
    for e in range(sr.n_par(n_in)):
        assert math.fsum(tw[:, e]) == math.fsum(td[:, e]), e
    pred, t = sr.errors_case(B, 1)
    sw, _ = wr.error_sums_ref(pred[0], t, wt)
    d = t.astype(np.float64) - pred[0]
    for o in range(4):
        dd, tt = np.append(d[o], d[o, k]), np.append(t[o], t[o, k]).astype(np.float64)
        ref = [math.fsum(dd * dd), math.fsum(np.abs(dd)), math.fsum(dd), math.fsum(np.abs(tt)), np.max(np.abs(dd)), np.max(np.abs(tt))]
        if sr._LONG:                                                         # (extended precision: both sides are that sum rounded once)
            assert np.allclose(sw[o], ref, rtol=2.0 ** -50, atol=0)
        else:
            assert list(sw[o]) == ref
    zero = wr.error_sums_ref(pred[0], t, np.where(np.arange(B) == B - 1, 0.0, 1.0))[0]
    assert zero[1, 4] < 1000.0 and zero[1, 5] < 1000.0                        # errors_case's outlier sits at the last index: it left


def test_weighted_replay_at_weight_one_is_the_unweighted_replay_bit_for_bit():
    import torch
    x, y = sr.raw_samples(400, 5, 3)
    sets = sr.host_sets(x, y, 3)
    ones = (np.ones(len(sets[0][0])), np.ones(len(sets[1][0])))
    wa, ha = wr.replay(torch.float64, sets, ones, 3, 64, 2)
    wb, hb = sr.replay(torch.float64, sets, 3, 64, 2)
    assert np.array_equal(wa, wb)
    for k in sr.SERIES:
        assert ha[k] == hb[k], k


def test_column_split_follows_the_preshuffle():
    from miniweatherml_amd import surrogate_train as st
    n, seed = 257, 12
    n_train, n_val, n_test = st.split_sizes(n)
    parts = wr.split_column(np.arange(n, dtype=np.float32), seed, n_train, n_val)
    assert [len(p) for p in parts] == [n_train, n_val, n_test]
    assert np.array_equal(np.concatenate(parts).astype(np.int64), st.preshuffle_permutation(n, seed))
    x, y = sr.raw_samples(n, 5, 1)
    x[:, 0] = np.arange(n)                                                   # the column travels with its sample (host_sets scales x0 to i / (n - 1))
    sets = sr.host_sets(x, y, seed)
    for k in range(3):
        assert np.array_equal(np.rint(sets[k][0][:, 0].astype(np.float64) * (n - 1)).astype(np.int64), parts[k].astype(np.int64))


def test_planted_and_log_uniform_weights():
    w = wr.planted_weights(300)
    assert list(np.flatnonzero(w != 1)) == [0, 63, 64, 255, 256, 299] and list(w[[0, 63, 64, 255, 256, 299]]) == [16, 0, 16, 0, 16, 0]
    assert list(wr.planted_weights(1)) == [16.0] and list(wr.planted_weights(65)[[0, 63, 64]]) == [16, 0, 16]
    u = wr.log_uniform_weights(8192, 0)
    assert u.dtype == np.float32 and u.min() >= 2.0 ** -4 and u.max() <= 2.0 ** 4 and abs(np.log2(u).mean()) < 0.1


def test_direction_holds_in_the_fp64_replay_by_a_factor():
    """The end-to-end direction test asserts an ordering on the GPU; here the weighted fp64 replay shows it for the same data and seed with
    a margin: continued with file weights (1, 16), the (1, 1) model's unweighted test loss on file B ends at least three times lower than
    continued with (1, 1) (measured: 1.8e-2 against 2.8e-3, a factor 6.6)."""
    plain, heavy = wr.direction_replay()
    print("file B test loss after the continuation: weights (1, 1) %.4e, (1, 16) %.4e, factor %.2f" % (plain, heavy, plain / heavy))
    assert heavy * 3.0 <= plain
