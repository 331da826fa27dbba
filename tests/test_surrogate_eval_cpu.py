"""The surrogate evaluator without a GPU: the C ABI's table, the loud failure of the device entry points, what SurrogateBank refuses, the
files behind `surrogate_train --keep-all`, and the arithmetic of SurrogateEvaluator.report / combine on hand-made results."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mw_surrogate_bank_create", "mw_surrogate_bank_destroy", "mw_surrogate_eval_group", "mw_surrogate_eval")


def shipped():
    from miniweatherml_amd import modules
    return modules.load_surrogate_weights()


def stencil_net(seed=0):
    from miniweatherml_amd import surrogate_train as st
    W1, b1, W2, b2, si, so = shipped()
    w = st.split_weights(st.initial_weights(seed, 1, stencil=True)[0])
    si9 = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]]))
    return np.ascontiguousarray(w[0]), w[1].copy(), np.ascontiguousarray(w[2]), w[3].copy(), si9, so


def test_header_binding_table_and_exports_agree(mw):
    from miniweatherml_amd import capi
    header = open(os.path.join(ROOT, "include", "mw_cdna4.h")).read()
    L = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert int(re.search(r"#define MW_SURROGATE_MAX_MODELS (\d+)", header).group(1)) == capi.MW_SURROGATE_MAX_MODELS


def test_kernels_are_no_dispatcher_family(mw):
    """The coverage gate of tests/conftest.py counts the dispatcher's kernel families only: the evaluator's kernels are in the library under
    names of their own."""
    import conftest
    from miniweatherml_amd import capi
    names = set()
    for m in re.finditer(rb"_ZN2mw(\d+)([0-9A-Za-z_]+)\.kd\x00", open(capi.LIB_PATH, "rb").read()):
        names.add(m.group(2)[:int(m.group(1))].decode())
    new = {"k_surrogate_eval", "k_surrogate_eval_stencil", "k_surrogate_eval_strict", "k_surrogate_eval_final", "k_surrogate_bank_recip"}
    assert new <= names and not (new & conftest._DISPATCHED)


def test_entry_points_fail_loudly_without_gpu(mw):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    W1, b1, W2, b2, si, so = shipped()
    params = np.concatenate([W1.ravel(), b1, W2.ravel(), b2]).astype(np.float32)
    h = C.c_void_p()
    # argument checks first, then "no HIP device"
    assert L.mw_surrogate_bank_create(C.byref(h), 6, 1, params.ctypes.data_as(fp), si.ctypes.data_as(dp), so.ctypes.data_as(dp)) != 0
    assert b"n_in must be 5" in L.mw_last_error()
    assert L.mw_surrogate_bank_create(C.byref(h), 5, 1, params.ctypes.data_as(fp), si.ctypes.data_as(dp), so.ctypes.data_as(dp)) != 0
    assert b"no HIP device" in L.mw_last_error() and h.value is None
    fields = (C.c_void_p * 5)(*([0x1000] * 5))
    assert L.mw_surrogate_eval(C.c_void_p(0x1000), 4, 16, fields, fields, C.c_void_p(0x1000), C.c_void_p(0x1000), None) != 0
    assert b"no HIP device" in L.mw_last_error()
    assert L.mw_surrogate_eval(C.c_void_p(0x1000), 0, 16, fields, fields, C.c_void_p(0x1000), C.c_void_p(0x1000), None) != 0
    assert b"nz and ncol" in L.mw_last_error()
    assert L.mw_surrogate_eval(None, 4, 16, fields, fields, C.c_void_p(0x1000), C.c_void_p(0x1000), None) != 0
    assert b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval_group(None) == 0 and b"null handle" in L.mw_last_error()
    L.mw_surrogate_bank_destroy(None)
    with pytest.raises(capi.MWError, match="no HIP device"):
        modules.SurrogateBank([shipped()])


def test_bank_refuses_bad_model_lists(mw):
    from miniweatherml_amd import capi, modules
    one, nine = shipped(), stencil_net()
    with pytest.raises(capi.MWError, match="different widths"):
        modules.SurrogateBank([one, nine, one])
    with pytest.raises(capi.MWError, match="no models"):
        modules.SurrogateBank([])
    with pytest.raises(capi.MWError, match="at most %d" % capi.MW_SURROGATE_MAX_MODELS):
        modules.SurrogateBank([one] * (capi.MW_SURROGATE_MAX_MODELS + 1))
    with pytest.raises(capi.MWError, match="scaling tables"):
        modules.SurrogateBank([one[:4] + (nine[4], one[5])])


def parent_weights_text(w, n_in):
    """weights.txt as the trainer has always written it: four titled blocks of repr(float(fp32 value)) lines."""
    a = 10 * n_in
    out = []
    for title, lo, hi in (("dense_6 kernel (%d,10) row-major" % n_in, 0, a), ("dense_6 bias (10)", a, a + 10),
                          ("dense_7 kernel (10,4) row-major", a + 10, a + 50), ("dense_7 bias (4)", a + 50, a + 54)):
        out.append("# %s\n" % title)
        out.extend(repr(float(x)) + "\n" for x in np.asarray(w, np.float32)[lo:hi])
    return "".join(out)


@pytest.mark.parametrize("stencil", [False, True])
def test_keep_all_files_round_trip(mw, tmp_path, stencil):
    """write_outputs(..., all_weights=): weights_<k>.txt for every model beside the best model's files; load_surrogate_bank returns the
    same fp32 values; weights.txt and the scaling files are byte for byte what the call without all_weights writes."""
    from miniweatherml_amd import modules, surrogate_train as st
    n_in = 9 if stencil else 5
    w = st.initial_weights(3, 4, stencil=stencil)
    w[:, -4:] = np.float32(0.1) * np.arange(1, 5, dtype=np.float32)           # (a fresh draw's biases are zero)
    rng = np.random.default_rng(2)
    scl_in = np.sort(rng.uniform(0.0, 300.0, (n_in, 2)), axis=1)
    scl_out = np.sort(rng.uniform(0.0, 300.0, (4, 2)), axis=1)
    best = 2
    plain = st.write_outputs(str(tmp_path / "plain"), w[best], scl_in, scl_out, {"a": 1})
    paths, models = st.write_outputs(str(tmp_path / "all"), w[best], scl_in, scl_out, {"a": 1}, all_weights=w, names=["s%d" % k for k in range(4)])
    assert [os.path.basename(p) for p in paths] == [os.path.basename(p) for p in plain] == ["weights.txt", "input_scaling.txt", "output_scaling.txt"]
    for a, b in zip(plain, paths):
        assert open(a, "rb").read() == open(b, "rb").read()
    assert open(paths[0]).read() == parent_weights_text(w[best], n_in)
    assert open(tmp_path / "all" / "history.json").read() == open(tmp_path / "plain" / "history.json").read()
    assert sorted(os.listdir(tmp_path / "plain")) == ["history.json", "input_scaling.txt", "output_scaling.txt", "weights.txt"]
    assert sorted(os.listdir(tmp_path / "all")) == ["history.json", "input_scaling.txt", "output_scaling.txt", "weights.txt"] + ["weights_%d.txt" % k for k in range(4)]
    assert [m["name"] for m in models] == ["s0", "s1", "s2", "s3"]
    assert all(set(m) == {"name", "keras_weights_txt", "nn_input_scaling", "nn_output_scaling"} for m in models)
    nets = modules.load_surrogate_bank(models)
    for k, net in enumerate(nets):
        assert net[0].shape == (n_in, 10) and net[0].dtype == np.float32
        assert np.array_equal(np.concatenate([net[0].ravel(), net[1], net[2].ravel(), net[3]]), w[k])
        assert np.array_equal(net[4], scl_in) and np.array_equal(net[5], scl_out)
    assert open(models[best]["keras_weights_txt"], "rb").read() == open(paths[0], "rb").read()
    with pytest.raises(st.SurrogateTrainError, match="all_weights"):
        st.write_outputs(str(tmp_path / "bad"), w[best], scl_in, scl_out, {}, all_weights=w[:, :50])


def test_driver_reads_the_model_list(mw, tmp_path):
    from miniweatherml_amd import driver, surrogate_train as st
    w = st.initial_weights(0, 2)
    W1, b1, W2, b2, si, so = shipped()
    _, models = st.write_outputs(str(tmp_path / "t"), w[0], si, so, {}, all_weights=w)
    base = ("sim_time: 10\nnx_glob: 8\nny_glob: 8\nnz: 8\nxlen: 1\nylen: 1\nzlen: 1\ndt_phys: 0\nout_prefix: x\ninit_data: supercell\nout_freq: -1\n")
    lst = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in m.items()) for m in models)
    p = tmp_path / "in.yaml"
    p.write_text(base + lst + "eval_interval: 3\n")
    assert driver.surrogate_config(driver.load_config(str(p))) == (models, 3)
    p.write_text(base + lst)
    assert driver.surrogate_config(driver.load_config(str(p))) == (models, 1)
    p.write_text(base + lst.replace("model_1", "model_0"))
    with pytest.raises(ValueError, match="unique"):
        driver.surrogate_config(driver.load_config(str(p)))
    p.write_text(base + lst.replace("weights_1.txt", "nothing.txt"))
    driver.load_config(str(p))                                   # another experiment's YAML may carry a stale list: nobody looks
    with pytest.raises(FileNotFoundError):
        driver.surrogate_config(driver.load_config(str(p)))
    p.write_text(base + "surrogate_models: []\n")
    with pytest.raises(ValueError, match="non-empty"):
        driver.surrogate_config(driver.load_config(str(p)))
    p.write_text(base)
    with pytest.raises(KeyError, match="surrogate_models"):
        driver.surrogate_config(driver.load_config(str(p)))
    assert "evaluate_surrogates" in driver.EXPERIMENTS


class FakeBank:
    def __init__(self, models, n_in=5):
        self.models, self.n_in = models, n_in


def random_raw(rng, k, empty=None):
    stats = rng.uniform(-1.0, 1.0, (k + 1, 2, 4, 4)) * 10.0 ** rng.integers(-12, 6, (k + 1, 2, 4, 4))
    stats[..., 1:] = np.abs(stats[..., 1:])
    counts = rng.integers(1, 10 ** 6, 2).astype(np.int64)
    if empty is not None:
        stats[:, empty] = 0.0
        counts[empty] = 0
    return stats, counts


def test_report_arithmetic(mw):
    """report() on a hand-made (K + 1, 2, 4, 4) array: n, bias, mae, rmse, max_abs and rmse / the persistence row's rmse, per class and for
    both classes together; an empty class gives n = 0 and no division by zero."""
    from miniweatherml_amd import modules
    k = 2
    stats = np.zeros((k + 1, 2, 4, 4))
    for m in range(k + 1):
        for c in range(2):
            for v in range(4):
                stats[m, c, v] = [(-1) ** v * (m + 1) * (c + 2) * 0.5, (m + 1) * (c + 2) * 1.5, (m + 1) ** 2 * (c + 1) * 9.0, (m + 1) * (v + c + 1.0)]
    counts = np.array([6, 10], dtype=np.int64)
    ev = modules.SurrogateEvaluator([FakeBank(k)], ["a", "b"])
    ev.total = [modules.surrogate_scores(stats, counts)]
    rep = ev.report()
    assert list(rep) == ["a", "b", "persistence:0"]
    for m, name in enumerate(rep):
        for c, cname in enumerate(("inactive", "active")):
            row = rep[name][cname]
            assert row["n"] == counts[c]
            for v, f in enumerate(modules.EVAL_FIELDS):
                s = stats[m, c, v]
                want = {"bias": s[0] / counts[c], "mae": s[1] / counts[c], "rmse": math.sqrt(s[2] / counts[c]), "max_abs": s[3],
                        "rmse_over_persistence": math.sqrt(s[2] / counts[c]) / math.sqrt(stats[k, c, v, 2] / counts[c])}
                assert row[f] == pytest.approx(want, rel=1e-15), (name, cname, f)
        row = rep[name]["all"]
        assert row["n"] == 16
        for v, f in enumerate(modules.EVAL_FIELDS):
            s = stats[m, 0, v] + stats[m, 1, v]
            assert row[f]["bias"] == pytest.approx(s[0] / 16, rel=1e-15) and row[f]["mae"] == pytest.approx(s[1] / 16, rel=1e-15)
            assert row[f]["rmse"] == pytest.approx(math.sqrt(s[2] / 16), rel=1e-15) and row[f]["max_abs"] == max(stats[m, 0, v, 3], stats[m, 1, v, 3])
    assert rep["persistence:0"]["active"]["temp"]["rmse_over_persistence"] == 1.0
    assert rep["a"]["all"]["temp"]["rmse_over_persistence"] == pytest.approx(1.0 / 3.0, rel=1e-15)
    # an empty class, and a persistence row without error
    stats2, counts2 = stats.copy(), np.array([0, 10], dtype=np.int64)
    stats2[:, 0] = 0.0
    stats2[k, 1, 3] = 0.0                                         # persistence is exact on precip_liquid
    ev.total = [modules.surrogate_scores(stats2, counts2)]
    with np.errstate(all="raise"):
        rep = ev.report()
    assert rep["a"]["inactive"]["n"] == 0 and all(x is None for x in rep["a"]["inactive"]["temp"].values())
    assert rep["a"]["active"]["precip_liquid"]["rmse_over_persistence"] is None and rep["a"]["active"]["precip_liquid"]["rmse"] > 0
    assert rep["a"]["all"]["temp"]["rmse"] == rep["a"]["active"]["temp"]["rmse"]
    assert "persistence:0" in ev.table(rep)
    with pytest.raises(modules.MWError, match="names"):
        modules.SurrogateEvaluator([FakeBank(2)], ["a"])


def test_combine_is_associative_and_exact(mw):
    """Sums are exact integers (units of 2^-1074): (a + b) + c and a + (b + c) are the same numbers, whatever the magnitudes; maxima and
    counts likewise.  The float a report sees is the correctly rounded exact sum."""
    from fractions import Fraction
    from miniweatherml_amd import modules
    rng = np.random.default_rng(8)
    raws = [random_raw(rng, 3), random_raw(rng, 3, empty=0), random_raw(rng, 3)]
    a, b, c = [[modules.surrogate_scores(s, n)] for s, n in raws]
    comb = modules.SurrogateEvaluator.combine
    left, right = comb(comb(a, b), c), comb(a, comb(b, c))
    other = comb(comb(c, a), b)
    for x, y in ((left, right), (left, other)):
        assert np.array_equal(x[0]["sums"], y[0]["sums"]) and np.array_equal(x[0]["max"], y[0]["max"])
        assert np.array_equal(x[0]["counts"], y[0]["counts"]) and x[0]["calls"] == y[0]["calls"] == 3
    assert np.array_equal(left[0]["counts"], raws[0][1] + raws[1][1] + raws[2][1])
    assert np.array_equal(left[0]["max"], np.maximum(np.maximum(raws[0][0][..., 3], raws[1][0][..., 3]), raws[2][0][..., 3]))
    got = modules._sums_to_float(left[0]["sums"], left[0]["nonfinite"])
    for idx in np.ndindex(got.shape):
        exact = sum(Fraction(float(r[0][idx])) for r in raws)
        assert got[idx] == float(exact), idx
    # a diverged model: its sum stays inf, the others stay exact
    bad = raws[0][0].copy()
    bad[1, 1, 2, 2] = np.inf
    d = comb([modules.surrogate_scores(bad, raws[0][1])], b)
    f = modules._sums_to_float(d[0]["sums"], d[0]["nonfinite"])
    assert f[1, 1, 2, 2] == np.inf and f[0, 1, 2, 2] == raws[0][0][0, 1, 2, 2] + raws[1][0][0, 1, 2, 2]
    with pytest.raises(modules.MWError, match="different"):
        comb(a, a + a)
