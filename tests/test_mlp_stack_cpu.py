"""The files of a dense surrogate stack (mlp.write_surrogate_stack / load_surrogate_stack) and who refuses them: no GPU."""
import re

import numpy as np
import pytest


def a_stack(form="state", n_in=5, widths=(7, 3)):
    from miniweatherml_amd import mlp
    rng = np.random.default_rng(11)
    w = [n_in] + list(widths) + [4]
    layers = [(rng.standard_normal((a, b)).astype(np.float32), rng.standard_normal(b).astype(np.float32)) for a, b in zip(w[:-1], w[1:])]
    return mlp.SurrogateStack(layers, np.array([0.1, 1.0 / 3.0][:len(widths)], np.float32), rng.standard_normal((n_in, 2)) * 1e3,
                              rng.standard_normal((4, 2)) / 3.0, form)


@pytest.mark.parametrize("form", ["state", "tendency"])
@pytest.mark.parametrize("n_in", [5, 9])
def test_round_trip_keeps_the_bits(tmp_path, form, n_in):
    from miniweatherml_amd import mlp
    s = a_stack(form, n_in)
    t = mlp.load_surrogate_stack(*mlp.write_surrogate_stack(s, str(tmp_path)))
    assert t.form == form and mlp.stack_widths(t) == [n_in, 7, 3, 4]
    for (W, b), (V, c) in zip(s.layers, t.layers):
        assert V.dtype == np.float32 and W.tobytes() == V.tobytes() and b.tobytes() == c.tobytes()
    assert s.slopes.tobytes() == t.slopes.tobytes() and s.scl_in.tobytes() == t.scl_in.tobytes() and s.scl_out.tobytes() == t.scl_out.tobytes()


def rewritten(path, old, new):
    text = open(path).read()
    assert old in text
    open(path, "w").write(text.replace(old, new, 1))


@pytest.mark.parametrize("case", ["no header", "no slopes", "count", "slope count", "width", "input rows", "output rows"])
def test_mismatched_files_are_refused_by_name(tmp_path, case):
    from miniweatherml_amd import capi, mlp
    w, si, so = mlp.write_surrogate_stack(a_stack(), str(tmp_path))
    edit, named = {"no header": ((w, "# stack:", "# shape:"), w), "no slopes": ((w, "# slopes:", "# slope:"), w),
                   "count": ((w, "# stack: 5 7 3 4", "# stack: 5 7 4 4"), w), "slope count": ((w, "# slopes: ", "# slopes: 0.5 "), w),
                   "width": ((w, "# stack: 5 7 3 4", "# stack: 5 65 3 4"), w),
                   "input rows": ((si, "\n", "\n1.0 2.0\n"), si), "output rows": ((so, "\n", "\n1.0 2.0\n"), so)}[case]
    rewritten(*edit)
    with pytest.raises(capi.MWError, match=re.escape(named)):
        mlp.load_surrogate_stack(w, si, so)


def test_the_fixed_model_loaders_and_the_banks_refuse_a_stack_file(tmp_path):
    from miniweatherml_amd import capi, driver, mlp
    w, si, so = mlp.write_surrogate_stack(a_stack(), str(tmp_path))
    with pytest.raises(capi.MWError, match="load_surrogate_stack"):
        mlp.load_surrogate_model(w, si, so)
    entry = {"name": "wide", "keras_weights_txt": w, "nn_input_scaling": si, "nn_output_scaling": so}
    with pytest.raises(ValueError, match="inference_ponni only"):
        driver._surrogate_models([entry], str(tmp_path))
