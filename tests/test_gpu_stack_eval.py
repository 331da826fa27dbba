"""mw_stack_group_eval / mlp.MlpStackGroup.evaluate: groups of dense stacks scored against the truth fields.

The reference is plain: a stack's prediction is MlpStack.forward's (a separately tested path) on the same state, out of place; the 32
numbers are numpy fp64 with math.fsum for the sums.  Bounds, derived: max |d| and the counts are exact (a maximum has no order,
persistence's d is one fp64 subtraction); a sum S of n terms x_i of any summation tree differs from the exactly rounded one by at most
n * 2^-53 * fsum(|x_i|), with the terms d * d of sum d^2 rounded to fp64 as the kernel rounds them."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BEFORE = (0, 2, 3, 4)                      # the input field that output v replaces
LO = np.array([200.0, 0.2, 0.0, 0.0, 0.0])
HI = np.array([320.0, 1.3, 0.02, 0.003, 0.006])
FIVE = ((5, (1,), "state"), (9, (10,), "tendency"), (5, (17,), "tendency"), (9, (17, 5), "state"), (5, (32,), "state"))
GROUPS = {"one": ((5, (17,), "state"),),
          "two_wide": ((5, (64,) * 4, "tendency"), (5, (64,) * 4, "state")),
          "two_stencil": ((9, (10,), "state"), (9, (17, 5), "tendency")),
          "five": FIVE}


def a_stack(n_in, widths, form):
    """A stack whose scaling tables are the state's ranges and whose weights depend on its shape and form alone."""
    from miniweatherml_amd import mlp
    rng = np.random.default_rng([n_in, len(form)] + list(widths))
    w = [n_in] + list(widths) + [4]
    layers = [((rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32), rng.uniform(-0.1, 0.1, b).astype(np.float32)) for a, b in zip(w[:-1], w[1:])]
    rows = list(range(5)) + [0, 2, 3, 4][:n_in - 5]
    scl_out = np.stack([LO[list(BEFORE)], HI[list(BEFORE)]], axis=1) * (1.0 if form == "state" else 1e-2)
    return mlp.SurrogateStack(layers, np.full(len(widths), 0.1, np.float32), np.stack([LO[rows], HI[rows]], axis=1), scl_out, form)


_STATES = {}


def state(nz, ncol, nan_cell=None):
    """(in5, truth4) on the GPU, computed once per shape: inputs uniform over [LO, HI], truth = input on about half the cells and input +
    1e-3 .. 1e-2 of the field's range, either sign, on the others."""
    import torch
    key = (nz, ncol, nan_cell)
    if key not in _STATES:
        rng = np.random.default_rng(nz * 1000003 + ncol)
        ins = [rng.uniform(LO[i], HI[i], (nz, ncol)) for i in range(5)]
        act = rng.random((nz, ncol)) < 0.5
        truth = [np.where(act, ins[b] + rng.uniform(1e-3, 1e-2, (nz, ncol)) * (HI[b] - LO[b]) * rng.choice([-1.0, 1.0], (nz, ncol)), ins[b]) for b in BEFORE]
        if nan_cell is not None:
            ins[0][nan_cell] = np.nan
        _STATES[key] = tuple([torch.from_numpy(a).cuda() for a in arrs] for arrs in (ins, truth))
    return _STATES[key]


def reference(preds, in5, truth4):
    """(stats (2, 4, 4), bound (2, 4, 3), counts) of four predicted fields; NaN where a class holds one (eval_max's semantics)."""
    before = [in5[b].cpu().numpy().ravel() for b in BEFORE]
    truth = [t.cpu().numpy().ravel() for t in truth4]
    act = np.zeros(truth[0].shape, bool)
    for v in range(4):
        act |= np.abs(truth[v] - before[v]) > 1e-10
    stats, bound = np.zeros((2, 4, 4)), np.zeros((2, 4, 3))
    counts = np.array([np.count_nonzero(~act), np.count_nonzero(act)], dtype=np.int64)
    for c, sel in enumerate((~act, act)):
        for v in range(4):
            d = (preds[v].cpu().numpy().ravel() - truth[v])[sel]
            terms = (d, np.abs(d), d * d)
            stats[c, v, :3] = [math.fsum(t) for t in terms]
            stats[c, v, 3] = np.nan if np.isnan(d).any() else np.max(np.abs(d), initial=0.0)
            bound[c, v] = [counts[c] * 2.0 ** -53 * math.fsum(np.abs(t)) for t in terms]
    return stats, bound, counts


def check_group(specs, nz, ncol, strict, nan_cell=None):
    """One group's evaluate against the reference rows (the stacks in the caller's order, then persistence); returns (stats, counts)."""
    from miniweatherml_amd import mlp
    in5, truth4 = state(nz, ncol, nan_cell)
    stacks = [a_stack(*s) for s in specs]
    group = mlp.MlpStackGroup(stacks, "cuda:0")
    group.strict = strict
    got, counts = group.evaluate(nz, in5, truth4)
    assert got.shape == (len(specs) + 1, 2, 4, 4)
    preds = [mlp.MlpStack(s, "cuda:0").forward(nz, *in5, strict=strict) for s in stacks] + [[in5[b] for b in BEFORE]]
    for m, pred in enumerate(preds):
        stats, bound, cnt = reference(pred, in5, truth4)
        assert np.array_equal(counts, cnt) and cnt.min() > 0, (m, counts, cnt)
        assert np.array_equal(got[m, :, :, 3], stats[:, :, 3], equal_nan=True), (m, "max", got[m, :, :, 3], stats[:, :, 3])
        assert np.array_equal(np.isnan(got[m]), np.isnan(stats)), (m, got[m], stats)
        ok = ~np.isnan(stats[:, :, :3])
        err = np.abs(got[m, :, :, :3] - stats[:, :, :3])[ok]
        print("row %d: worst |sum - fsum| / bound = %.3g" % (m, np.max(err / np.where(bound[ok] > 0, bound[ok], 1.0), initial=0.0)))
        assert np.all(err <= bound[ok]), (m, err, bound[ok])
    return got, counts


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("name", list(GROUPS))
def test_small_shapes_against_the_forward(mw, name, strict):
    """nz = 5, ncol = 17: a partial cell tile, a partial column tile, nz no multiple of the four levels per pass; groups with mpb = 1
    (four waves, four slots), mpb = 1 with grid.y = 2 (two images that do not share the LDS), mpb = 2, and both lists with mpb = 4, an
    idle wave and rows in the caller's order."""
    check_group(GROUPS[name], 5, 17, strict)


def test_a_second_grid_stride_pass(mw):
    """grid.x is at most 1024 blocks of four slots, so some slot makes a second pass once the flat walk has more than 4096 tile quads
    (more than 4096 * 4 * 16 = 262144 cells) and the column walk more than 4096 column tiles (more than 65536 columns): nz = 4 and
    ncol = 65537 is the smallest shape with both (262148 cells)."""
    check_group(((5, (17,), "tendency"), (9, (10,), "state")), 4, 65537, 0)


def test_a_row_does_not_depend_on_the_group(mw):
    """Nine blocks of the flat walk, five of the column walk: every stack of the five alone gives its row's bits, the persistence row
    and the counts are the same in every group, and a second call repeats the first."""
    from miniweatherml_amd import mlp
    nz, ncol = 7, 300
    in5, truth4 = state(nz, ncol)
    group = mlp.MlpStackGroup([a_stack(*s) for s in FIVE], "cuda:0")
    got, counts = group.evaluate(nz, in5, truth4)
    again, counts2 = group.evaluate(nz, in5, truth4)
    assert got.tobytes() == again.tobytes() and np.array_equal(counts, counts2)
    for j, spec in enumerate(FIVE):
        alone, c1 = mlp.MlpStackGroup([a_stack(*spec)], "cuda:0").evaluate(nz, in5, truth4)
        assert alone[0].tobytes() == got[j].tobytes(), (j, alone[0], got[j])
        assert alone[1].tobytes() == got[-1].tobytes() and np.array_equal(c1, counts), j


@pytest.mark.parametrize("strict", [0, 1])
def test_nan_reaches_its_class_alone(mw, strict):
    """temp of one input cell is NaN: the reference rows (NaN in the sums and the maximum of that cell's class, in the stacks' rows and in
    persistence) hold with equal_nan, and the other class stays finite."""
    got, _ = check_group(FIVE, 5, 17, strict, nan_cell=(2, 5))
    assert np.isnan(got[:, :, 0, :]).any(axis=(1, 2)).all()                # every row shows it in temp ...
    single = [j for j, s in enumerate(FIVE) if s[0] == 5] + [len(FIVE)]    # ... and in one class where the cell is the row's only reader
    assert (np.isnan(got[single]).any(axis=(2, 3)).sum(axis=1) == 1).all() # (n_in = 9: the cell below reads it too)


def test_driver_scores_stacks(mw, tmp_path, monkeypatch):
    """evaluate_surrogates on a 16 x 12 x 10 supercell, two steps, one fixed model and one stack: the stack is listed under `stacks`, its
    report rows are finite and cover every cell; a second run with the stack alone and no surrogate_models reports too."""
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from miniweatherml_amd import driver, mlp
    entries, _ = write_models(tmp_path)
    w, si, so = mlp.write_surrogate_stack(a_stack(9, (17, 5), "tendency"), str(tmp_path / "deep"))
    line = lambda e: "  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items())      # noqa: E731
    stacks = "surrogate_stacks:\n" + line({"name": "deep", "keras_weights_txt": w, "nn_input_scaling": si, "nn_output_scaling": so})
    monkeypatch.chdir(tmp_path)
    for extra, models, bank, reported in (("surrogate_models:\n" + line(entries[0]) + stacks, ["single_a"], 1, {"single_a", "persistence:0", "deep", "persistence:1"}),
                                         (stacks, [], 0, {"deep", "persistence:0"})):
        path, _ = write_yaml(tmp_path, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
        driver.run("evaluate_surrogates", path, max_steps=2, quiet=True)
        doc = json.load(open(os.path.join(str(tmp_path), "surrogate_evaluation.json")))
        assert [m["name"] for m in doc["models"]] == models and set(doc["report"]) == reported
        assert [(s["name"], s["bank"], s["widths"], s["form"]) for s in doc["stacks"]] == [("deep", bank, [9, 17, 5, 4], "tendency")]
        assert doc["stacks"][0]["slopes"] == pytest.approx([0.1, 0.1])
        row = doc["report"]["deep"]["all"]
        assert row["n"] == 2 * 16 * 12 * 10
        assert all(np.isfinite(row[f]["rmse"]) and np.isfinite(row[f]["max_abs"]) for f in ("temp", "water_vapor", "cloud_liquid", "precip_liquid"))
