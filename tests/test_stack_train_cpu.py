"""Host side of the stack trainer (miniweatherml_amd/surrogate_train.py), no GPU: what is refused before
anything reaches the device, the layer list of a stack and its parameter count."""
import numpy as np
import pytest

from test_surrogate_train_cpu import write_sample_file


def _init_dirs(tmp_path):
    """A stack 5 -> 8 -> 4 with slope 0.1 in one directory, the shipped fixed model's layout in another."""
    from miniweatherml_amd import mlp, surrogate_train as st
    scl_in, scl_out = np.array([[0.0, 1.0]] * 5), np.array([[0.0, 1.0]] * 4)
    w = st.stack_initial_weights(0, 1, [5, 8, 4])[0]
    mlp.write_surrogate_stack(mlp.SurrogateStack(st.split_stack_weights(w, [5, 8, 4]), [0.1], scl_in, scl_out, "state"), str(tmp_path / "stack"))
    st.write_outputs(str(tmp_path / "fixed"), st.initial_weights(0, 1)[0], scl_in, scl_out, {})
    return str(tmp_path / "stack"), str(tmp_path / "fixed")


REFUSALS = [("width0", dict(stack=[0]), ("width", "[1, 64]")), ("width65", dict(stack=[32, 65]), ("width", "65")),
            ("depth0", dict(stack=[]), ("depth", "[1, 4]")), ("depth5", dict(stack=[8] * 5), ("depth", "5")),
            ("slope_count", dict(stack=[8, 8], slopes=[0.1, 0.1, 0.1]), ("3 slopes", "2 hidden")),
            ("slope_negative", dict(stack=[8], slopes=-0.1), ("slope", ">= 0")), ("slope_nan", dict(stack=[8], slopes=[float("nan")]), ("slope", "finite")),
            ("committee", None, ("--committee", "--stack")),
            ("init_other_shape", dict(stack=[8, 8], init="stack"), ("init", "same shape")), ("init_other_slope", dict(stack=[8], slopes=0.2, init="stack"), ("init", "slopes")),
            ("init_fixed", dict(stack=[8], init="fixed"), ("init", "fixed model")), ("fixed_from_stack", dict(init="stack"), ("init", "dense stack"))]


@pytest.mark.parametrize("name,kw,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_stack_refusals_on_the_host(tmp_path, capsys, name, kw, words):
    from miniweatherml_amd import surrogate_train as st
    rng = np.random.default_rng(0)
    path = tmp_path / "s.nc"
    write_sample_file(path, [(rng.random((40, 5, 2), dtype=np.float32), rng.random((40, 4), dtype=np.float32))])
    if kw is None:
        assert st.main([str(path), "--out", str(tmp_path / "o"), "--stack", "8", "--keep-all", "--committee"]) == 2
        msg = capsys.readouterr().err
    else:
        dirs = dict(zip(("stack", "fixed"), _init_dirs(tmp_path)))
        if "init" in kw:
            kw = dict(kw, init=dirs[kw["init"]])
        with pytest.raises(st.SurrogateTrainError) as e:
            st.train_surrogate([str(path)], None, device="cpu", **kw)
        msg = str(e.value)
    assert all(w in msg for w in words), msg


@pytest.mark.parametrize("widths,slopes,npar", [([5, 10, 4], [0.1], 104), ([9, 17, 3, 4], [0.0, 0.25], 240), ([9, 64, 64, 64, 64, 4], [0.1] * 4, 13380)])
def test_stack_layer_list_and_parameter_count(widths, slopes, npar):
    from miniweatherml_amd import surrogate_train as st
    assert st.stack_n_params(widths) == npar
    lay, off, width = st.stack_layers(widths, slopes), 0, widths[0]
    assert len(lay) == 3 * (len(widths) - 1) - 1
    for kind, n_i, n_o, slope, o in lay:                                  # a chain: Matvec (W at its offset), Bias, Relu with the layer's slope
        assert n_i == width
        if kind == 0:
            assert o == off
            off += n_i * n_o
        elif kind == 1:
            assert o == off and n_o == n_i
            off += n_o
        else:
            assert slope == slopes[[l for l in lay if l[0] == 2].index((kind, n_i, n_o, slope, o))]
        width = n_o
    assert off == npar and width == 4
    assert st._layers(5) == ((0, 5, 10, 0.0, 0), (1, 10, 10, 0.0, 50), (2, 10, 10, 0.1, 0), (0, 10, 4, 0.0, 60), (1, 4, 4, 0.0, 100))
