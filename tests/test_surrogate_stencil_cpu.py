"""The two-cell stencil surrogate (9 -> 10 -> 4), the parts that run without a GPU: the sample reader's column order, the host statement
of the feature order (modules.stencil_features), the seeded initial weights, the output files and the loader's refusals."""
import json
import os

import numpy as np
import pytest

from test_surrogate_train_cpu import write_sample_file


def stencil_chunks(rng, sizes, hole=np.nan):
    """Random sample chunks in DataGenerator's layout; inputs[:, 4, 1] (slot 1 has four variables: DataGenerator never assigns its
    fifth row) holds `hole`."""
    out = []
    for n in sizes:
        a = rng.random((n, 5, 2), dtype=np.float32)
        a[:, 4, 1] = hole
        out.append((a, rng.random((n, 4), dtype=np.float32)))
    return out


def test_read_samples_stencil_column_order(mw, tmp_path):
    """Columns 0..4 = slot 0, columns 5..8 = rows 0, 1, 2, 3 of slot 1; the unassigned [4, 1] entry (NaN in this file) is never read,
    so the data passes the finiteness check; the default call is the single-cell reader, unchanged."""
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(0)
    chunks = stencil_chunks(rng, [700, 0, 301])
    path = write_sample_file(tmp_path / "s.nc", chunks)
    ins = np.concatenate([c[0] for c in chunks])
    outs = np.concatenate([c[1] for c in chunks])
    x9, y9, meta = st.read_samples([path], stencil=True)
    assert x9.shape == (1001, 9) and x9.dtype == np.float32 and y9.shape == (1001, 4)
    for col, (row, slot) in enumerate([(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (1, 1), (2, 1), (3, 1)]):
        assert np.array_equal(x9[:, col], ins[:, row, slot]), col
    assert np.isfinite(x9).all() and np.array_equal(y9, outs)
    si, so = st.data_scaling(x9, y9)
    assert si.shape == (9, 2) and so.shape == (4, 2)
    assert np.array_equal(si[:, 0], x9.min(0).astype(np.float64)) and np.array_equal(si[:, 1], x9.max(0).astype(np.float64))
    x5, y5, meta5 = st.read_samples([path])
    assert x5.shape == (1001, 5) and np.array_equal(x5, ins[:, :, 0]) and np.array_equal(y5, outs)
    assert meta["time_step_size"] == meta5["time_step_size"] == 0.5
    assert len(st.STENCIL_IN_NAMES) == 9 and st.STENCIL_IN_NAMES[:5] == st.IN_NAMES


def test_constant_stencil_feature_is_refused(mw, tmp_path):
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(1)
    chunks = stencil_chunks(rng, [50], hole=0.0)
    chunks[0][0][:, 2, 1] = 0.25                                      # cloud liquid of the level above: feature 7
    path = write_sample_file(tmp_path / "c.nc", chunks)
    x9, y9, _ = st.read_samples([path], stencil=True)
    with pytest.raises(st.SurrogateTrainError, match=r"input variable 7 \(cloud liquid density \(level above\)\) is constant"):
        st.data_scaling(x9, y9)
    st.data_scaling(*st.read_samples([path])[:2])                     # the single-cell model does not see it


def loop_features(fields, nz, ny, nx, nens):
    """The feature order written out cell by cell (generate_micro_surrogate_data.h:139-156 on the coupler's (nz, ny, nx, nens) arrays)."""
    out = np.empty((9, nz, ny, nx, nens))
    for k in range(nz):
        ka = min(nz - 1, k + 1)
        for j in range(ny):
            for i in range(nx):
                for e in range(nens):
                    here = [f[k, j, i, e] for f in fields]
                    above = [fields[v][ka, j, i, e] for v in (0, 2, 3, 4)]
                    out[:, k, j, i, e] = here + above
    return out.reshape(9, -1)


@pytest.mark.parametrize("shape", [(1, 3, 4, 1), (2, 1, 5, 1), (5, 3, 2, 3), (4, 2, 3, 2)])
def test_stencil_features_order(mw, shape):
    from miniweatherml_amd import modules
    nz, ny, nx, nens = shape
    rng = np.random.default_rng(nz * 100 + nens)
    fields = [rng.random(shape) + 10.0 * v for v in range(5)]
    X = modules.stencil_features(fields, nz)
    assert X.shape == (9, nz * ny * nx * nens)
    assert np.array_equal(X, loop_features(fields, nz, ny, nx, nens))
    top = X.reshape(9, nz, -1)[:, nz - 1]
    assert np.array_equal(top[5:], top[[0, 2, 3, 4]])                 # the top level's "level above" is the level itself
    assert np.array_equal(X, modules.stencil_features([f.reshape(nz, -1) for f in fields], nz))     # flat columns: the same
    if nens > 1 and nz > 1:                                           # the ensemble members do not mix
        f2 = [f.copy() for f in fields]
        for f in f2:
            f[..., 1] += 100.0
        X2 = modules.stencil_features(f2, nz).reshape(9, nz, ny, nx, nens)
        assert np.array_equal(X2[..., 0], X.reshape(9, nz, ny, nx, nens)[..., 0])
    with pytest.raises(Exception):
        modules.stencil_features(fields[:4], nz)


def test_initial_weights_stencil(mw):
    """144 draws from the same seeded streams: uniform [-0.05, 0.05) kernels, zero biases, model m of K = seed + m alone."""
    from miniweatherml_amd import surrogate_train as st
    w = st.initial_weights(7, 3, stencil=True)
    assert w.shape == (3, 144) and w.dtype == np.float32 and st.n_params(True) == 144 and st.n_params() == 104
    W1, b1, W2, b2 = st.split_weights(w[1])
    assert W1.shape == (9, 10) and W2.shape == (10, 4) and not b1.any() and not b2.any()
    ker = np.concatenate([W1.ravel(), W2.ravel()])
    assert ker.min() >= -0.05 and ker.max() < 0.05 and len(np.unique(ker)) == 130
    assert np.array_equal(st.initial_weights(8, 1, stencil=True)[0], w[1])
    assert st.initial_weights(7, 1).shape == (1, 104)                 # the default is the single-cell model


def test_stencil_output_files_round_trip(mw, tmp_path):
    """144 values, 9 scaling rows, history.json; read back bitwise by load_surrogate_weights, which infers the model from the counts."""
    from miniweatherml_amd import modules, surrogate_train as st
    rng = np.random.default_rng(2)
    w = (rng.standard_normal(144) * rng.choice([1e-6, 1e-2, 1.0, 30.0], 144)).astype(np.float32)
    si = np.sort(rng.random((9, 2)).astype(np.float32), axis=1).astype(np.float64)
    so = np.sort(rng.random((4, 2)).astype(np.float32), axis=1).astype(np.float64)
    paths = st.write_outputs(str(tmp_path / "o"), w, si, so, {"inputs": "stencil"})
    assert len(np.loadtxt(paths[0], comments="#")) == 144 and np.loadtxt(paths[1]).shape == (9, 2) and np.loadtxt(paths[2]).shape == (4, 2)
    assert json.load(open(os.path.join(str(tmp_path / "o"), "history.json")))["inputs"] == "stencil"
    W1, b1, W2, b2, si2, so2 = modules.load_surrogate_weights(weights_txt=paths[0], in_scaling_txt=paths[1], out_scaling_txt=paths[2])
    assert W1.shape == (9, 10) and b1.shape == (10,) and W2.shape == (10, 4) and b2.shape == (4,) and W1.dtype == np.float32
    assert np.array_equal(np.concatenate([W1.ravel(), b1, W2.ravel(), b2]), w)
    assert np.array_equal(si2, si) and np.array_equal(so2, so) and si2.shape == (9, 2)
    for a, b in zip(st.split_weights(w), (W1, b1, W2, b2)):
        assert np.array_equal(a, b)
    # the single-cell files still load as before, and the default is the shipped single-cell model
    p5 = st.write_outputs(str(tmp_path / "o5"), w[:104], si[:5], so, {})
    assert modules.load_surrogate_weights(weights_txt=p5[0], in_scaling_txt=p5[1], out_scaling_txt=p5[2])[0].shape == (5, 10)
    assert modules.load_surrogate_weights()[0].shape == (5, 10)
    with pytest.raises(st.SurrogateTrainError, match="9 input scaling rows with 104 weights"):
        st.write_outputs(str(tmp_path / "bad"), w[:104], si, so, {})


def test_mismatched_surrogate_files_are_refused(mw, tmp_path):
    """Scaling rows and weight counts that do not belong to one model; the message names both counts.  A stencil scaling table beside
    an .h5 weight file (always the single-cell model) is refused as well."""
    from miniweatherml_amd import modules, surrogate_train as st
    from miniweatherml_amd.capi import MWError
    rng = np.random.default_rng(3)
    w = rng.standard_normal(144).astype(np.float32)
    si = np.sort(rng.random((9, 2)), axis=1)
    so = np.sort(rng.random((4, 2)), axis=1)
    p9 = st.write_outputs(str(tmp_path / "nine"), w, si, so, {})
    p5 = st.write_outputs(str(tmp_path / "five"), w[:104], si[:5], so, {})
    seven = str(tmp_path / "seven.txt")
    np.savetxt(seven, si[:7])
    short = str(tmp_path / "short.txt")
    np.savetxt(short, w[:100])
    h5 = os.path.join(os.path.dirname(modules.__file__), "data", "supercell_kessler_singlecell_model_weights.h5")
    for kw, rows, nw in ((dict(weights_txt=p9[0], in_scaling_txt=p5[1]), 5, 144), (dict(weights_txt=p5[0], in_scaling_txt=p9[1]), 9, 104),
                         (dict(weights_txt=p5[0], in_scaling_txt=seven), 7, 104), (dict(weights_txt=short, in_scaling_txt=p9[1]), 9, 100),
                         (dict(weights_txt=p9[0]), 5, 144), (dict(weights_h5=h5, in_scaling_txt=p9[1]), 9, 104)):
        with pytest.raises(MWError, match="%d input scaling rows with %d weights" % (rows, nw)):
            modules.load_surrogate_weights(out_scaling_txt=p9[2], **kw)


def test_stencil_cli_and_arguments(mw, tmp_path, capsys):
    """--stencil exists; the host-side refusals are those of the single-cell trainer (no device is touched before them)."""
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(4)
    path = write_sample_file(tmp_path / "s.nc", stencil_chunks(rng, [40]))
    with pytest.raises(st.SurrogateTrainError, match="batch_size"):
        st.train_surrogate([path], batch_size=0, stencil=True)
    assert st.main([path, "--out", str(tmp_path / "o"), "--stencil", "--epochs", "0"]) == 2
    assert "epochs must be an integer >= 1" in capsys.readouterr().err
