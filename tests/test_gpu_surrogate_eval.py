"""mw_surrogate_eval on the GPU: a bank of candidate networks scored against a truth state, per output field and per active / inactive
class, next to the persistence baseline.

The reference of every comparison is the project's own forward (modules.mlp_forward / mlp_stencil_forward, or the numpy restatement of the
strict form) written to temporaries and reduced on the host: maxima and counts must be EQUAL, and every sum must lie within
n * 2^-52 * sum |terms| of the exactly rounded (math.fsum) sum of the same terms -- the bound of a fixed-order fp64 sum of n terms
(k_surrogate_sums).  That bound is only enough because the predictions inside the kernel carry the bits the
forward kernels store."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
BEFORE = (0, 2, 3, 4)                      # the input field that output v replaces


# ---- models -----------------------------------------------------------------------------------------------------------------------
def model_pool(n_in, count):
    """`count` models of one width with two different pairs of scaling tables (even / odd index): surrogate_train.initial_weights draws,
    and for n_in = 5 the shipped network as model 0 (n_in = 9: a network of the shipped one's magnitude with all nine rows alive)."""
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    if n_in == 9:
        rng = np.random.default_rng(1)
        W1 = np.ascontiguousarray(np.concatenate([W1, rng.permutation(W1[[0, 2, 3, 4]].ravel()).reshape(4, 10)]).astype(np.float32))
        si = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]] * np.array([[0.97, 1.02]])]))
    si_b = np.ascontiguousarray(si * np.array([[0.95, 1.04]]) + np.array([[0.0, 1e-4]]))      # (precip_liquid's min is 0: keep max > min)
    so_b = np.ascontiguousarray(so * np.array([[1.0, 1.1]]))
    pool = [(W1, b1, W2, b2, si, so)]
    draws = st.initial_weights(7, count - 1, stencil=(n_in == 9))
    for k in range(count - 1):
        w = st.split_weights(draws[k])
        # the biases of a fresh draw are zero: give them life, or a model is blind to the layers' C operands
        rng = np.random.default_rng(100 + k)
        b1k, b2k = rng.uniform(-0.05, 0.05, 10).astype(np.float32), rng.uniform(0.0, 0.5, 4).astype(np.float32)
        pool.append((np.ascontiguousarray(w[0]), b1k, np.ascontiguousarray(w[2]), b2k) + ((si_b, so_b) if k % 2 == 0 else (si, so)))
    return pool


_POOLS, _BANKS = {}, {}


def pool(n_in):
    from miniweatherml_amd import modules
    if n_in not in _POOLS:
        g = modules.SurrogateBank(model_pool(n_in, 1)).group
        _POOLS[n_in] = (model_pool(n_in, 2 * g + 1), g)
    return _POOLS[n_in]


def bank_of(n_in, idx):
    """A bank of the pool's models `idx` (cached: banks are uploaded once)."""
    from miniweatherml_amd import modules
    key = (n_in, tuple(idx))
    if key not in _BANKS:
        _BANKS[key] = modules.SurrogateBank([pool(n_in)[0][i] for i in idx])
    return _BANKS[key]


# ---- states -----------------------------------------------------------------------------------------------------------------------
def make_state(n_in, nz, ncol, seed, active="half"):
    """Nine host fields (nz, ncol): inputs uniform over the shipped scaling ranges; truth = input on the inactive cells and input + a
    perturbation of 1e-3 .. 1e-2 of the field's range (>> 1e-10, either sign, all four fields) on the active ones."""
    si = pool(n_in)[0][0][4]
    so = pool(n_in)[0][0][5]
    rng = np.random.default_rng(seed)
    ins = [rng.uniform(si[i, 0], si[i, 1], (nz, ncol)) for i in range(5)]
    act = {"half": rng.random((nz, ncol)) < 0.5, "all": np.ones((nz, ncol), bool), "none": np.zeros((nz, ncol), bool)}[active]
    truth = []
    for v in range(4):
        delta = rng.uniform(1e-3, 1e-2, (nz, ncol)) * (so[v, 1] - so[v, 0]) * rng.choice([-1.0, 1.0], (nz, ncol))
        truth.append(np.where(act, ins[BEFORE[v]] + delta, ins[BEFORE[v]]))
    return ins, truth


def to_gpu(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


# ---- host reference -----------------------------------------------------------------------------------------------------------------
def host_stats(pred, truth, ins):
    """(stats (2, 4, 4), bound (2, 4, 3), counts (2,)) of one prediction: exactly rounded sums of d, |d|, d^2 and the maximum of |d| per
    class and field; bound = n * 2^-52 * sum |terms| with n the cells of the class."""
    pred, truth = [np.ravel(p) for p in pred], [np.ravel(t) for t in truth]
    before = [np.ravel(ins[i]) for i in BEFORE]
    act = np.zeros(truth[0].shape, bool)
    for v in range(4):
        act |= np.abs(truth[v] - before[v]) > 1e-10
    stats, bound = np.zeros((2, 4, 4)), np.zeros((2, 4, 3))
    counts = np.array([np.count_nonzero(~act), np.count_nonzero(act)], dtype=np.int64)
    for c, sel in enumerate((~act, act)):
        for v in range(4):
            d = (pred[v] - truth[v])[sel]
            for s, terms in enumerate((d, np.abs(d), d * d)):
                stats[c, v, s] = math.fsum(terms)
            stats[c, v, 3] = np.max(np.abs(d)) if d.size else 0.0
            # sum |terms|: of d and of |d| it is the exact sum of |d| itself, of d^2 the exact sum of d^2
            bound[c, v] = counts[c] * 2.0 ** -52 * stats[c, v, [1, 1, 2]]
    return stats, bound, counts


def np_strict_forward(X, net):
    """The restatement of tests/test_gpu_surrogate_stencil.py (np_stencil_forward) on a feature matrix X (n_in, cells) of either width:
    fp32 in index order, one rounding per operation, the quotient form of the scaling."""
    W1, b1, W2, b2, si, so = net
    x = ((X - si[:, 0:1]) / (si[:, 1:2] - si[:, 0:1])).astype(np.float32)
    W1, b1, W2, b2 = [np.asarray(a, np.float32) for a in (W1, b1, W2, b2)]
    h = []
    for o in range(10):
        acc = np.zeros(x.shape[1], np.float32)
        for i in range(x.shape[0]):
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


def reference_rows(n_in, nz, ins, truth, strict):
    """host_stats of every model of the pool (and of persistence, last) on one state, from the existing forward's temporaries."""
    from miniweatherml_amd import modules
    models, _ = pool(n_in)
    t = to_gpu(ins)
    rows = []
    for net in models:
        if strict:
            X = modules.stencil_features(ins, nz) if n_in == 9 else np.stack([np.ravel(a) for a in ins])
            pred = np_strict_forward(X, net)
        elif n_in == 9:
            pred = [o.cpu().numpy() for o in modules.mlp_stencil_forward(nz, *t, *net)]
        else:
            pred = [o.cpu().numpy() for o in modules.mlp_forward(*t, *net)]
        rows.append(host_stats(pred, truth, ins))
    rows.append(host_stats([ins[i] for i in BEFORE], truth, ins))
    return rows


def check_rows(got, counts, want_rows, what):
    """got (K + 1, 2, 4, 4) and counts against host_stats results (K models, then persistence)."""
    for m, (stats, bound, cnt) in enumerate(want_rows):
        assert np.array_equal(counts, cnt), (what, m, counts, cnt)
        assert np.array_equal(got[m, :, :, 3], stats[:, :, 3]), (what, m, "max", got[m, :, :, 3], stats[:, :, 3])
        err = np.abs(got[m, :, :, :3] - stats[:, :, :3])
        print("%s row %d: worst |sum - fsum| / bound = %.3g" % (what, m, np.max(err / np.where(bound > 0, bound, 1.0))))
        assert np.all(err <= bound), (what, m, err, bound)


def k_values(g):
    return (1, 2, g, g + 1, 2 * g + 1)


def run_case(n_in, nz, ncol, strict):
    ins, truth = make_state(n_in, nz, ncol, seed=1000 * nz + ncol)
    rows = reference_rows(n_in, nz, ins, truth, strict)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    g = pool(n_in)[1]
    for k in k_values(g):
        bank = bank_of(n_in, range(k))
        assert bank.group == g and bank.models == k
        bank.strict = int(strict)
        got, counts = bank.evaluate(nz, tin, ttr)
        bank.strict = 0
        assert got.shape == (k + 1, 2, 4, 4) and counts.dtype == np.int64
        check_rows(got, counts, rows[:k] + rows[-1:], "n_in %d (%d, %d) K %d strict %d" % (n_in, nz, ncol, k, strict))
        # the persistence row of this input: exactly zero on the inactive cells (input == truth there)
        assert np.all(got[k, 0] == 0.0)


CELLS5 = [1, 15, 16, 17, 31, 32, 33, 261, 70001]
SHAPES9 = [(1, 1), (2, 17), (7, 16), (8, 15), (9, 33), (17, 40), (33, 16)]


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("ncells", CELLS5)
def test_single_cell_bank_against_the_forward(mw, ncells, strict):
    """n_in = 5, K in {1, 2, G, G + 1, 2G + 1}: the tail of a 16-cell tile, several tiles per wave, several waves, the grid-stride loop and
    a final pass over many blocks (70001 cells).  strict = 0: against mlp_forward's temporaries; 1: against the numpy restatement."""
    run_case(5, 1, ncells, strict)


# z chunks of k_mlp_stencil's rule that each stencil shape must produce: (number of chunks, the last one shorter)
CHUNKS9 = {(1, 1): (1, False), (2, 17): (1, False), (7, 16): (1, False), (8, 15): (1, False), (9, 33): (2, True), (17, 40): (3, True),
           (33, 16): (5, True)}


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", SHAPES9)
def test_stencil_bank_against_the_forward(mw, shape, strict):
    """n_in = 9: a level that is its own level above (nz = 1, the top), one / two / three and more z chunks with a short last one (asserted
    through mw_mlp_stencil_chunk), column tails."""
    from miniweatherml_amd import capi
    nz, ncol = shape
    zc = capi.lib().mw_mlp_stencil_chunk(nz, ncol)
    assert ((nz + zc - 1) // zc, nz % zc != 0) == CHUNKS9[shape], (shape, zc)
    run_case(9, nz, ncol, strict)


@pytest.mark.parametrize("n_in", [5, 9])
def test_class_edge_and_empty_classes(mw, n_in):
    """before = 0.0, after = 1e-10 exactly: inactive; after = nextafter(1e-10, 1): active (strictly greater, gather_micro_statistics.h:61-74).
    All-active and all-inactive states: counts (0, n) and (n, 0) with zeros in the empty class."""
    nz, ncol = 3, 37
    n = nz * ncol
    ins, truth = make_state(n_in, nz, ncol, seed=5, active="none")
    ins[3][...] = 0.0                                                  # cloud_liquid before
    edge = np.full((nz, ncol), 1e-10)
    over = np.zeros((nz, ncol), bool)
    over.ravel()[::3] = True
    edge[over] = np.nextafter(1e-10, 1.0)
    truth[2] = edge
    bank = bank_of(n_in, range(2))
    got, counts = bank.evaluate(nz, to_gpu(ins), to_gpu(truth))
    assert counts.tolist() == [n - int(over.sum()), int(over.sum())]
    assert got[2, 0, 2, 3] == 1e-10 and got[2, 1, 2, 3] == np.nextafter(1e-10, 1.0)       # persistence, max |d| of cloud_liquid per class
    for active, want in (("all", [0, n]), ("none", [n, 0])):
        ins, truth = make_state(n_in, nz, ncol, seed=6, active=active)
        got, counts = bank.evaluate(nz, to_gpu(ins), to_gpu(truth))
        assert counts.tolist() == want
        empty = 0 if active == "all" else 1
        assert np.all(got[:, empty] == 0.0) and np.all(got[:2, 1 - empty, :, 1] > 0.0)


@pytest.mark.parametrize("n_in,shape", [(5, (1, 70001)), (9, (17, 40))])
def test_rows_do_not_depend_on_the_bank(mw, n_in, shape):
    """One model alone, first, last, and on both sides of a pass boundary (positions G - 1, G, 2G) of a bank of 2G + 1: the same bytes, and
    the same bytes from two identical calls."""
    nz, ncol = shape
    ins, truth = make_state(n_in, nz, ncol, seed=77)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    g = pool(n_in)[1]
    target = 3
    alone, counts = bank_of(n_in, [target]).evaluate(nz, tin, ttr)
    again, counts2 = bank_of(n_in, [target]).evaluate(nz, tin, ttr)
    assert alone.tobytes() == again.tobytes() and counts.tobytes() == counts2.tobytes()
    others = [i for i in range(2 * g + 1) if i != target]
    for pos in (0, g - 1, g, 2 * g):
        idx = others[:pos] + [target] + others[pos:]
        got, cnt = bank_of(n_in, idx).evaluate(nz, tin, ttr)
        assert got[pos].tobytes() == alone[0].tobytes(), pos
        assert got[-1].tobytes() == alone[-1].tobytes() and cnt.tobytes() == counts.tobytes()


class _OneState:
    """What Microphysics_Kessler_Surrogate.mean_diffs reads of a coupler."""
    def __init__(self, fields):
        import torch
        self.fields, self.device = fields, torch.device("cuda:0")

    def get_data_manager_readonly(self):
        return self

    def get(self, name, readonly=False):
        return self.fields[name]


@pytest.mark.parametrize("n_in,shape", [(5, (1, 4099)), (9, (9, 333))])
def test_agrees_with_the_mean_diff_prints(mw, n_in, shape):
    """(sum d of class 0 + sum d of class 1) / n is the module's `Relative diff` (mean_diffs, microphysics_kessler_ponni.h:266-269) of the same
    model and fields, within the bound of the sums over n: n * 2^-52 * sum |d| / n, with sum |d| the host's exact sum over the forward's
    temporaries."""
    from miniweatherml_amd import modules
    nz, ncol = shape
    n = nz * ncol
    ins, truth = make_state(n_in, nz, ncol, seed=9)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    net = pool(n_in)[0][0]
    micro = modules.Microphysics_Kessler_Surrogate.__new__(modules.Microphysics_Kessler_Surrogate)
    micro._nn_out = modules.mlp_stencil_forward(nz, *tin, *net) if n_in == 9 else modules.mlp_forward(*tin, *net)
    diffs = micro.mean_diffs(_OneState(dict(zip(("temp", "water_vapor", "cloud_liquid", "precip_liquid"), ttr))))
    got, _ = bank_of(n_in, [0]).evaluate(nz, tin, ttr)
    for v, key in enumerate(("temp", "rho_v", "rho_c", "rho_r")):
        sum_abs = math.fsum(np.abs(micro._nn_out[v].cpu().numpy().ravel() - truth[v].ravel()))
        bound = n * 2.0 ** -52 * sum_abs / n
        err = abs((got[0, 0, v, 0] + got[0, 1, v, 0]) / n - diffs[key])
        print("%s: |mean - mean_diffs| / bound = %.3g" % (key, err / bound))
        assert err <= bound, (key, diffs[key], err, bound)


@pytest.mark.parametrize("n_in,strict", [(5, 0), (9, 0), (5, 1), (9, 1)])
def test_nothing_is_written_to_the_fields(mw, n_in, strict):
    nz, ncol = 9, 333
    ins, truth = make_state(n_in, nz, ncol, seed=4)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    bank = bank_of(n_in, range(3))
    bank.strict = strict
    bank.evaluate(nz, tin, ttr)
    bank.strict = 0
    for t, a in zip(tin + ttr, ins + truth):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_entry_point_errors(mw):
    from miniweatherml_amd import capi
    L = capi.lib()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    net = pool(5)[0][0]
    params = np.concatenate([np.ravel(a) for a in net[:4]]).astype(np.float32)
    si, so = net[4].copy(), net[5].copy()
    h = C.c_void_p()
    args = (params.ctypes.data_as(fp), si.ctypes.data_as(dp), so.ctypes.data_as(dp))
    assert L.mw_surrogate_bank_create(C.byref(h), 7, 1, *args) != 0 and b"n_in must be 5" in L.mw_last_error()
    assert L.mw_surrogate_bank_create(C.byref(h), 5, 0, *args) != 0 and b"models must be in" in L.mw_last_error()
    assert L.mw_surrogate_bank_create(C.byref(h), 5, capi.MW_SURROGATE_MAX_MODELS + 1, *args) != 0 and b"models must be in" in L.mw_last_error()
    assert L.mw_surrogate_bank_create(C.byref(h), 5, 1, None, args[1], args[2]) != 0 and b"null pointer" in L.mw_last_error()
    bad = si.copy()
    bad[2, 1] = bad[2, 0]
    assert L.mw_surrogate_bank_create(C.byref(h), 5, 1, args[0], bad.ctypes.data_as(dp), args[2]) != 0 and b"max == min" in L.mw_last_error()
    assert h.value is None
    bank = bank_of(5, [0])
    ins, truth = make_state(5, 1, 16, seed=1)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    from miniweatherml_amd.modules import _field_ptr_array
    out = to_gpu([np.zeros(66)])[0]
    a5, a4 = _field_ptr_array(tin), _field_ptr_array(ttr)
    optr, cptr = C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8 * 64)
    assert L.mw_surrogate_eval(bank._h, 0, 16, a5, a4, optr, cptr, None) != 0 and b"nz and ncol" in L.mw_last_error()
    assert L.mw_surrogate_eval(None, 1, 16, a5, a4, optr, cptr, None) != 0 and b"null pointer" in L.mw_last_error()
    assert L.mw_surrogate_eval(bank._h, 1, 16, a5, a4, None, cptr, None) != 0 and b"null pointer" in L.mw_last_error()
    a4[2] = None
    assert L.mw_surrogate_eval(bank._h, 1, 16, a5, a4, optr, cptr, None) != 0 and b"null field" in L.mw_last_error()


def test_bank_lives_on_one_device(mw):
    """The handle's buffers are on the bank's device: fields from elsewhere are refused before anything is launched."""
    import torch
    from miniweatherml_amd import modules
    from miniweatherml_amd.capi import MWError
    bank = bank_of(5, [0])
    assert bank.device == torch.device("cuda:0")
    ins, truth = make_state(5, 1, 33, seed=2)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    with pytest.raises(MWError, match="the bank lives on cuda:0"):
        bank.evaluate(1, [t.cpu() for t in tin], ttr)
    if torch.cuda.device_count() > 1:
        with pytest.raises(MWError, match="the bank lives on cuda:0"):
            bank.evaluate(1, tin, [t.to("cuda:1") for t in ttr])
        other = modules.SurrogateBank([pool(5)[0][0]], "cuda:1")
        got1, cnt1 = other.evaluate(1, [t.to("cuda:1") for t in tin], [t.to("cuda:1") for t in ttr])
        got0, cnt0 = bank.evaluate(1, tin, ttr)
        assert got1.tobytes() == got0.tobytes() and cnt1.tobytes() == cnt0.tobytes()


@pytest.mark.parametrize("n_in,strict", [(5, 0), (9, 0), (5, 1), (9, 1)])
def test_a_diverged_model_shows_nan_not_a_finite_maximum(mw, n_in, strict):
    """A NaN bias of the temperature output: that model's temperature sums AND maxima are NaN in both classes, its other fields and the
    other rows keep their bytes; report() flags the field and the history holds no bare NaN token."""
    from miniweatherml_amd import modules
    nz, ncol = 5, 37
    ins, truth = make_state(n_in, nz, ncol, seed=3)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    nets = [pool(n_in)[0][i] for i in range(3)]
    b2 = nets[1][3].copy()
    b2[0] = np.nan
    sick = modules.SurrogateBank([nets[0], nets[1][:3] + (b2,) + nets[1][4:], nets[2]])
    well = bank_of(n_in, range(3))
    sick.strict = well.strict = strict
    got, counts = sick.evaluate(nz, tin, ttr)
    ref, _ = well.evaluate(nz, tin, ttr)
    well.strict = 0
    assert np.isnan(got[1, :, 0, :]).all()
    assert got[1, :, 1:].tobytes() == ref[1, :, 1:].tobytes() and got[[0, 2, 3]].tobytes() == ref[[0, 2, 3]].tobytes()
    ev = modules.SurrogateEvaluator([sick], ["a", "b", "c"])
    ev.total = [modules.surrogate_scores(got, counts)]
    rep = ev.report()
    assert rep["b"]["active"]["temp"]["finite"] is False and rep["b"]["active"]["temp"]["max_abs"] is None
    assert "finite" not in rep["b"]["active"]["water_vapor"] and "finite" not in rep["a"]["all"]["temp"]
    text = json.dumps({"r": rep, "h": modules.json_safe(got.tolist())}, allow_nan=False)
    assert '"nan"' in text


# ---- evaluator class and driver -----------------------------------------------------------------------------------------------------
def write_models(tmp_path):
    """Three models of both widths as files: (entries of a surrogate_models list, the loaded tuples)."""
    from miniweatherml_amd import modules, surrogate_train as st
    entries = []
    for name, n_in, k in (("single_a", 5, 0), ("stencil_a", 9, 1), ("single_b", 5, 2)):
        net = pool(n_in)[0][k]
        d = str(tmp_path / name)
        paths = st.write_outputs(d, np.concatenate([np.ravel(a) for a in net[:4]]), net[4], net[5], {})
        entries.append({"name": name, "keras_weights_txt": paths[0], "nn_input_scaling": paths[1], "nn_output_scaling": paths[2]})
    return entries, modules.load_surrogate_bank(entries)


def same_result(a, b):
    return all(np.array_equal(x["sums"], y["sums"]) and np.array_equal(x["max"], y["max"]) and np.array_equal(x["counts"], y["counts"])
               and x["calls"] == y["calls"] for x, y in zip(a, b)) and len(a) == len(b)


def test_evaluator_accumulates_what_combine_gives(mw, tmp_path):
    """Two accumulate calls on different states equal combine of the two single-call results exactly, in either grouping with a third."""
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    entries, nets = write_models(tmp_path)
    banks = [modules.SurrogateBank([nets[0], nets[2]]), modules.SurrogateBank([nets[1]])]
    ev = modules.SurrogateEvaluator(banks, ["single_a", "single_b", "stencil_a"])
    coupler, dycore, micro = modules.make_supercell(16, 12, 10, 1, 8000., 6000., 20000.)
    singles = []
    for step in range(3):
        dt = dycore.compute_time_step(coupler)
        dycore.time_step(coupler, dt)
        dm = coupler.get_data_manager_readwrite()
        dm.get("cloud_liquid").add_(1e-4 * (step + 1))                 # something for Kessler to do
        inp = Coupler("cuda:0")
        coupler.clone_into(inp)
        micro.time_step(coupler, dt)
        singles.append(ev.accumulate(inp, coupler))
        if step == 1:
            assert same_result(ev.total, ev.combine(singles[0], singles[1]))
    assert same_result(ev.total, ev.combine(ev.combine(singles[0], singles[1]), singles[2]))
    assert same_result(ev.total, ev.combine(singles[0], ev.combine(singles[1], singles[2])))
    assert ev.total[0]["calls"] == 3 and int(ev.total[0]["counts"].sum()) == 3 * 16 * 12 * 10 and ev.total[0]["counts"][1] > 0
    rep = ev.report()
    assert set(rep) == {"single_a", "single_b", "stencil_a", "persistence:0", "persistence:1"}
    assert rep["persistence:0"]["all"]["temp"]["rmse_over_persistence"] == 1.0
    assert "single_b" in ev.table()


def test_driver_evaluate_surrogates(mw, tmp_path, monkeypatch):
    """driver.run("evaluate_surrogates") on a 16 x 12 x 10 grid with three models of both widths: the JSON's last call equals
    bank.evaluate on the states of a loop stepped by hand (the driver's own sequence of modules)."""
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver, modules
    from miniweatherml_amd.coupler import Coupler
    entries, nets = write_models(tmp_path)
    extra = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries) + "eval_interval: 2\n"
    path, _ = write_yaml(tmp_path, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
    monkeypatch.chdir(tmp_path)
    _, _, info = driver.run("evaluate_surrogates", path, max_steps=3, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_evaluation.json")))
    assert info["steps"] == 3 and [c["step"] for c in doc["history"]] == [0, 2]
    assert [m["name"] for m in doc["models"]] == ["single_a", "single_b", "stencil_a"] and [m["n_in"] for m in doc["models"]] == [5, 5, 9]
    assert set(doc["report"]) == {"single_a", "single_b", "stencil_a", "persistence:0", "persistence:1"}
    # the same loop by hand
    coupler, dycore, micro, nudger = modules.make_supercell(16, 12, 10, 1, 8000., 6000., 20000., with_nudger=True)
    banks = [modules.SurrogateBank([nets[0], nets[2]]), modules.SurrogateBank([nets[1]])]
    names5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
    for step in range(3):
        dt = dycore.compute_time_step(coupler)
        dycore.time_step(coupler, dt)
        inp = Coupler("cuda:0")
        coupler.clone_into(inp)
        micro.time_step(coupler, dt)
        if step == 2:
            in5 = [inp.get_data_manager_readonly().get(n, True) for n in names5]
            truth4 = [coupler.get_data_manager_readonly().get(n, True) for n in modules.EVAL_FIELDS]
            for ib, bank in enumerate(banks):
                stats, counts = bank.evaluate(10, in5, truth4)
                last = doc["history"][-1]["banks"][ib]
                assert np.array_equal(np.array(last["stats"]), stats) and last["counts"] == counts.tolist()
        modules.sponge_layer(coupler, dt)
        nudger.nudge_to_column(coupler, dt)


def test_driver_refuses_more_ranks(mw, tmp_path, monkeypatch):
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver
    entries, _ = write_models(tmp_path)
    extra = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    path, _ = write_yaml(tmp_path, nx=16, ny=12, nz=10, extra=extra)
    monkeypatch.setattr(driver, "_distributed", lambda device: (2, 0, device))
    with pytest.raises(ValueError, match="one rank"):
        driver.run("evaluate_surrogates", path, max_steps=1, quiet=True)
