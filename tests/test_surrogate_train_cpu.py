"""Surrogate training (miniweatherml_amd/surrogate_train.py), the parts that run without a GPU: the sample-file reader against the
independent reader tests/cdf.py, the split arithmetic, the permutations, the output files, the refusals, and the Nadam restatement
against torch.optim.NAdam (the oracle the GPU tests use)."""
import os

import numpy as np
import pytest

from cdf import Reader


def write_sample_file(path, chunks, dt=0.5, dx=500.0):
    """A file in DataGenerator's layout (modules.DataGenerator.init + generate_samples_stencil's appends): chunks = [(inputs (n, 5, 2),
    outputs (n, 4)), ...], appended one after the other."""
    from miniweatherml_amd import modules
    nc = modules._NcFile(str(path), True, 5)
    ds, dvi, dst, dvo = nc.def_dim("nsamples", 0), nc.def_dim("num_vars_in", 5), nc.def_dim("sten_size", 2), nc.def_dim("num_vars_out", 4)
    for n in ("time_step_size", "dx", "dy", "dz", "xlen", "ylen", "zlen"):
        nc.def_var_typed(n, 6, [])
    nc.def_var_typed("only_two_dimensions", 4, [])
    nc.def_var_typed("inputs", 5, [ds, dvi, dst])
    nc.def_var_typed("outputs", 5, [ds, dvo])
    nc.enddef()
    nc.close()
    nc = modules._NcFile(str(path), False)
    for name, val in (("time_step_size", dt), ("dx", dx), ("dy", dx), ("dz", 250.0), ("xlen", 1e5), ("ylen", 1e5), ("zlen", 2e4)):
        nc.put_typed(nc.varid(name), [], [], np.array([val], dtype=np.float64))
    nc.put_typed(nc.varid("only_two_dimensions"), [], [], np.array([1], dtype=np.int32))
    ul = 0
    for a, b in chunks:
        n = a.shape[0]
        if n:
            nc.put_typed(nc.varid("inputs"), [ul, 0, 0], [n, 5, 2], a.astype(np.float32))
            nc.put_typed(nc.varid("outputs"), [ul, 0], [n, 4], b.astype(np.float32))
            ul += n
            nc.set_numrecs(ul)
    nc.close()
    return str(path)


def random_chunks(rng, sizes):
    return [(rng.random((n, 5, 2), dtype=np.float32), rng.random((n, 4), dtype=np.float32)) for n in sizes]


def test_reader_matches_independent_reader(mw, tmp_path):
    from miniweatherml_amd import modules, surrogate_train as st
    rng = np.random.default_rng(1)
    f1 = write_sample_file(tmp_path / "a.nc", random_chunks(rng, [37, 0, 101, 5]))
    f2 = write_sample_file(tmp_path / "b.nc", random_chunks(rng, [64, 3]))
    for f in (f1, f2):
        nc = modules._NcFile(f, False)
        r = Reader(f)
        for name in ("inputs", "outputs", "time_step_size", "dx", "only_two_dimensions"):
            got, ref = nc.get(name), r.get(name)
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), name
        assert np.array_equal(nc.get("inputs", 10, 7), r.get("inputs")[10:17])
        nc.close()
    inputs, outputs, meta = st.read_samples([f1, f2])
    ref_in = np.concatenate([Reader(f).get("inputs")[:, :, 0] for f in (f1, f2)])
    ref_out = np.concatenate([Reader(f).get("outputs") for f in (f1, f2)])
    assert inputs.shape == (143 + 67, 5) and np.array_equal(inputs, ref_in) and np.array_equal(outputs, ref_out)
    assert meta["time_step_size"] == 0.5 and meta["dx"] == 500.0 and meta["dz"] == 250.0


@pytest.mark.parametrize("n", [3, 10, 1000, 20000, 9118906])
def test_split_sizes_follow_the_notebook(n):
    from miniweatherml_amd.surrogate_train import split_sizes
    n_fit = int((1 - 0.2) * n)
    assert split_sizes(n) == (int(n_fit * (1 - 0.2)), n_fit - int(n_fit * (1 - 0.2)), n - n_fit)
    if n == 9118906:
        assert split_sizes(n)[0] == 5836099
    if n == 20000:
        assert split_sizes(n) == (12800, 3200, 4000)
    assert split_sizes(1000, 0.3, 0.1) == (630, 70, 300)


@pytest.mark.parametrize("n", [1, 2, 5, 17, 1000, 65537])
def test_permutations_are_seeded_bijections(n):
    from miniweatherml_amd import surrogate_train as st
    for perm in (st.preshuffle_permutation(n, 7), st.epoch_permutation(n, 7, 2, 3)):
        assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(st.preshuffle_permutation(n, 7), st.preshuffle_permutation(n, 7))
    # model m of seed s is seed s + m (independent of how many models train together); epochs differ
    assert np.array_equal(st.epoch_permutation(n, 7, 2, 3), st.epoch_permutation(n, 9, 0, 3))
    if n >= 1000:
        assert not np.array_equal(st.epoch_permutation(n, 7, 0, 0), st.epoch_permutation(n, 7, 0, 1))
        assert not np.array_equal(st.preshuffle_permutation(n, 7), st.preshuffle_permutation(n, 8))
        assert not np.array_equal(st.preshuffle_permutation(n, 7), np.arange(n))


def test_initial_weights_are_keras_defaults_and_independent_of_k():
    from miniweatherml_amd.surrogate_train import initial_weights
    w4 = initial_weights(11, 4)
    assert w4.dtype == np.float32 and w4.shape == (4, 104)
    for m in range(4):
        assert np.array_equal(w4[m], initial_weights(11 + m, 1)[0])
    kern = np.concatenate([w4[:, :50], w4[:, 60:100]], axis=1)
    assert np.all(kern >= -0.05) and np.all(kern < 0.05) and np.std(kern) > 0.02
    assert not np.any(w4[:, 50:60]) and not np.any(w4[:, 100:])


def test_output_files_read_back_bitwise(mw, tmp_path):
    from miniweatherml_amd import modules, surrogate_train as st
    rng = np.random.default_rng(3)
    w = (rng.standard_normal(104) * rng.choice([1e-6, 1e-2, 1.0, 30.0], 104)).astype(np.float32)
    scl_in = np.sort(rng.random((5, 2)).astype(np.float32) * np.array([[300.0], [1.2], [0.02], [0.003], [0.01]], np.float32), axis=1)
    scl_out = np.sort(rng.random((4, 2)).astype(np.float32), axis=1)
    paths = st.write_outputs(str(tmp_path / "out"), w, scl_in.astype(np.float64), scl_out.astype(np.float64), {"x": 1})
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights(weights_txt=paths[0], in_scaling_txt=paths[1], out_scaling_txt=paths[2])
    got = np.concatenate([W1.ravel(), b1, W2.ravel(), b2])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), w.view(np.uint32))
    assert np.array_equal(si, scl_in.astype(np.float64)) and np.array_equal(so, scl_out.astype(np.float64))
    # the comment lines of the shipped weight file, in its order
    shipped = [ln for ln in open(os.path.join(os.path.dirname(modules.__file__), "data", "kessler_surrogate_weights.txt")) if ln.startswith("#")]
    assert [ln for ln in open(paths[0]) if ln.startswith("#")] == shipped
    assert os.path.exists(str(tmp_path / "out" / "history.json"))


def test_refusals_without_gpu(mw, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    E = st.SurrogateTrainError
    rng = np.random.default_rng(4)
    good = write_sample_file(tmp_path / "good.nc", random_chunks(rng, [200]))
    # constant variable, named
    a, b = random_chunks(rng, [50])[0]
    a[:, 3, 0] = 0.25
    const = write_sample_file(tmp_path / "const.nc", [(a, b)])
    with pytest.raises(E, match="cloud liquid density"):
        st.train_surrogate([const], device="cpu")
    a, b = random_chunks(rng, [50])[0]
    b[:, 1] = 0.0
    with pytest.raises(E, match="output variable 1 .water vapor density"):
        st.train_surrogate([write_sample_file(tmp_path / "const2.nc", [(a, b)])], device="cpu")
    # mixed time steps
    other = write_sample_file(tmp_path / "dt.nc", random_chunks(rng, [20]), dt=0.279)
    with pytest.raises(E, match="time_step_size"):
        st.train_surrogate([good, other], device="cpu")
    # empty file, non-finite values
    with pytest.raises(E, match="zero samples"):
        st.train_surrogate([write_sample_file(tmp_path / "empty.nc", [])], device="cpu")
    a, b = random_chunks(rng, [50])[0]
    a[7, 2, 0] = np.nan
    with pytest.raises(E, match="non-finite"):
        st.train_surrogate([write_sample_file(tmp_path / "nan.nc", [(a, b)])], device="cpu")
    a, b = random_chunks(rng, [50])[0]
    b[9, 0] = np.inf
    with pytest.raises(E, match="non-finite"):
        st.train_surrogate([write_sample_file(tmp_path / "inf.nc", [(a, b)])], device="cpu")
    # arguments
    for kw, msg in ((dict(test_split=0.0), "test_split"), (dict(test_split=1.0), "test_split"), (dict(validation_split=-0.1), "validation_split"),
                    (dict(validation_split=1.5), "validation_split"), (dict(batch_size=0), "batch_size"),
                    (dict(batch_size=st.MAX_BATCH + 1), "batch_size"), (dict(models=0), "models"), (dict(models=st.MAX_MODELS + 1), "models"),
                    (dict(epochs=0), "epochs"), (dict(test_split=0.999), "empty")):
        with pytest.raises(E, match=msg):
            st.train_surrogate([good], device="cpu", **kw)
    tiny = write_sample_file(tmp_path / "tiny.nc", random_chunks(rng, [2]))
    with pytest.raises(E, match="empty"):
        st.train_surrogate([tiny], device="cpu")
    with pytest.raises(E, match="no sample files"):
        st.train_surrogate([], device="cpu")


def nadam_restatement(w0, grad_fn, steps, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, decay=0.004):
    """The issue's formula in numpy fp64, with the product's per-step scalars (nadam_table in fp64)."""
    from miniweatherml_amd.surrogate_train import nadam_table
    tab = nadam_table(steps, lr, beta1, beta2, decay, dtype=np.float64)
    w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    for s in range(steps):
        g = grad_fn(w)
        m = beta1 * m + (1 - beta1) * g
        v = beta2 * v + (1 - beta2) * g * g
        w = w - (tab[s, 0] * g + tab[s, 1] * m) / (np.sqrt(v / tab[s, 2]) + eps)
    return w


def test_nadam_restatement_matches_torch_nadam():
    """The Nadam of the issue (TF 2.x Keras) is algebraically torch.optim.NAdam(eps=1e-7, momentum_decay=4e-3): 50 steps on a toy least
    squares problem agree to 1e-6 of the total weight change (not bitwise: torch keeps its step count, and so its schedule, in fp32)."""
    import torch
    rng = np.random.default_rng(5)
    A, b, w0 = rng.standard_normal((30, 20)), rng.standard_normal(30), rng.standard_normal(20) * 0.1
    w_np = nadam_restatement(w0, lambda w: 2 * A.T @ (A @ w - b) / len(b), 50)
    wt = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.NAdam([wt], lr=1e-3, betas=(0.9, 0.999), eps=1e-7, momentum_decay=4e-3)
    At, bt = torch.tensor(A), torch.tensor(b)
    for _ in range(50):
        opt.zero_grad()
        torch.mean((At @ wt - bt) ** 2).backward()
        opt.step()
    w_t = wt.detach().numpy()
    change = np.max(np.abs(w_t - w0))
    assert change > 1e-2
    assert np.max(np.abs(w_np - w_t)) <= 1e-6 * change
