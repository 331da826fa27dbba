"""mw_surrogate_eval_domain on the GPU: mw_surrogate_eval with every model's errors split by inside / outside the
model's training box.

Exact wherever possible.  With boxes nothing leaves (or nothing satisfies) a model's rows of one side are mw_surrogate_eval's bytes and the
other side is +0.0.  With general boxes the reference is tests/eval_domain_ref.py on the project's own forward (mlp_forward /
mlp_stencil_forward, or the numpy restatement of the strict form): counts and maxima EQUAL, every sum within n * 2^-52 * sum |terms| of
the exactly rounded sum, n the cells of the (side, class); a sum the reference finds NaN or infinite must be the same NaN or infinity."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import eval_domain_ref as ref

pytestmark = pytest.mark.gpu

BEFORE = ref.BEFORE
INF = np.inf
OPEN = np.array([[-INF, INF]] * 5)


# ---- models, boxes, banks -----------------------------------------------------------------------------------------------------------
def model_pool(n_in, count):
    """`count` state models of one width with two different pairs of scaling tables: the shipped network (n_in = 9: widened to nine live
    rows) and surrogate_train.initial_weights draws with biases of their own."""
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    if n_in == 9:
        rng = np.random.default_rng(1)
        W1 = np.ascontiguousarray(np.concatenate([W1, rng.permutation(W1[[0, 2, 3, 4]].ravel()).reshape(4, 10)]).astype(np.float32))
        si = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]] * np.array([[0.97, 1.02]])]))
    si_b = np.ascontiguousarray(si * np.array([[0.95, 1.04]]) + np.array([[0.0, 1e-4]]))
    so_b = np.ascontiguousarray(so * np.array([[1.0, 1.1]]))
    pool = [(W1, b1, W2, b2, si, so)]
    draws = st.initial_weights(11, count - 1, stencil=(n_in == 9))
    for k in range(count - 1):
        w = st.split_weights(draws[k])
        rng = np.random.default_rng(200 + k)
        b1k, b2k = rng.uniform(-0.05, 0.05, 10).astype(np.float32), rng.uniform(0.0, 0.5, 4).astype(np.float32)
        pool.append((np.ascontiguousarray(w[0]), b1k, np.ascontiguousarray(w[2]), b2k) + ((si_b, so_b) if k % 2 == 0 else (si, so)))
    return pool


E_MODEL = 3                                # the model whose box bounds density_dry alone: its outside-active class is empty by construction
_POOLS, _BANKS = {}, {}


def pool(n_in):
    """(models, g, boxes (2g + 1, 5, 2)): a different box per model inside the shipped input ranges.  Model 1: cloud_liquid and
    precip_liquid from lo = 0.0; model 2: temp and density_dry without an upper bound; model E_MODEL: density_dry alone."""
    from miniweatherml_amd import modules
    if n_in not in _POOLS:
        _POOLS[n_in] = build_pool(n_in, modules.SurrogateBank(model_pool(n_in, 1)).domain_group)
    return _POOLS[n_in]


def build_pool(n_in, g):
    models = model_pool(n_in, 2 * g + 1)
    si = models[0][4][:5]
    w = si[:, 1] - si[:, 0]
    boxes = np.empty((2 * g + 1, 5, 2))
    for m in range(2 * g + 1):
        boxes[m, :, 0] = si[:, 0] + (0.02 + 0.01 * (m % 5)) * w
        boxes[m, :, 1] = si[:, 1] - (0.03 + 0.01 * ((3 * m) % 5)) * w
    boxes[1, 3:, 0] = 0.0
    boxes[2, :2, 1] = INF
    boxes[E_MODEL] = OPEN
    boxes[E_MODEL, 1] = (si[1, 0] + 0.2 * w[1], si[1, 1] - 0.2 * w[1])
    return models, g, boxes


def bank_of(n_in, idx, forms=None):
    """A bank of the pool's models `idx` (cached: banks are uploaded once); forms: per model, default all state."""
    from miniweatherml_amd import modules
    key = (n_in, tuple(idx), tuple(forms) if forms else None)
    if key not in _BANKS:
        nets = [pool(n_in)[0][i] for i in idx]
        if forms:
            nets = [tuple(n) + (f,) for n, f in zip(nets, forms)]
        _BANKS[key] = modules.SurrogateBank(nets)
    return _BANKS[key]


def to_gpu(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in arrays]


# ---- states -------------------------------------------------------------------------------------------------------------------------
def make_state(n_in, nz, ncol, seed, plant="finite"):
    """Nine host fields (nz, ncol): inputs uniform over the shipped scaling ranges, half of the cells active (truth = input + 1e-3 .. 1e-2
    of the output's range, all four fields), density_dry of the active cells inside model E_MODEL's interval.  plant: values at model 0's
    (and 1's) bounds at level 0 and at the top, on inactive cells whose other fields sit at the centre of model 0's box:
      "finite"     lo, hi, one nextafter beyond each (temp, water_vapor), -0.0 (cloud_liquid, precip_liquid: lo = 0.0 of model 1)
      "nonfinite"  the same and NaN, +inf, -inf in density_dry (finite bounds of model 0, the infinite upper bound of model 2)
      None         nothing."""
    models, _, boxes = pool(n_in)
    si, so = models[0][4], models[0][5]
    rng = np.random.default_rng(seed)
    ins = [rng.uniform(si[i, 0], si[i, 1], (nz, ncol)) for i in range(5)]
    act = rng.random((nz, ncol)) < 0.5
    ins[1] = np.where(act, rng.uniform(boxes[E_MODEL, 1, 0], boxes[E_MODEL, 1, 1], (nz, ncol)), ins[1])
    planted = []
    if plant:
        b0 = boxes[0]
        items = [(f, x) for f in (0, 2) for x in (b0[f, 0], b0[f, 1], np.nextafter(b0[f, 0], -INF), np.nextafter(b0[f, 1], INF))]
        items += [(3, -0.0), (4, -0.0)]
        if plant == "nonfinite":
            items += [(1, np.nan), (1, INF), (1, -INF)]
        items = items[:max(1, ncol // 3)]                                    # (a narrow state keeps cells of its own; 39 columns hold all)
        for i, (f, x) in enumerate(items):
            for k, c in ((0, 3 * i % ncol), (nz - 1, (3 * i + 1) % ncol)):
                for q in range(5):
                    ins[q][k, c] = 0.5 * (b0[q, 0] + b0[q, 1])
                ins[f][k, c] = x
                act[k, c] = False
                planted.append((k, c, f, x))
    truth = []
    for v in range(4):
        delta = rng.uniform(1e-3, 1e-2, (nz, ncol)) * (so[v, 1] - so[v, 0]) * rng.choice([-1.0, 1.0], (nz, ncol))
        truth.append(np.where(act, ins[BEFORE[v]] + delta, ins[BEFORE[v]]))
    return ins, truth, planted


def predictions(n_in, nz, ins, strict, nets, forms=None):
    """Every net's four outputs on the state, from the project's own forward (strict: the numpy restatement)."""
    from miniweatherml_amd import modules
    t = to_gpu(ins)
    out = []
    for j, net in enumerate(nets):
        form = forms[j] if forms else "state"
        if strict:
            X = modules.stencil_features(ins, nz) if n_in == 9 else np.stack([np.ravel(a) for a in ins])
            out.append(ref.np_strict_forward(X, net, form))
        elif n_in == 9:
            out.append([o.cpu().numpy() for o in modules.mlp_stencil_forward(nz, *t, *net, form=form)])
        else:
            out.append([o.cpu().numpy() for o in modules.mlp_forward(*t, *net, form=form)])
    return out


def check_model(got, cnt, want, what):
    """One model's got (2, 2, 2, 4, 4) and cnt (2, 2) against eval_domain_ref.model_rows."""
    stats, bound, counts = want
    assert np.array_equal(cnt, counts), (what, cnt, counts)
    assert np.array_equal(got[..., 3], stats[..., 3], equal_nan=True), (what, "max", got[..., 3], stats[..., 3])
    g, w = got[..., :3], stats[..., :3]
    fin = np.isfinite(w)
    assert np.array_equal(g[~fin], w[~fin], equal_nan=True), (what, "non-finite sums", g[~fin], w[~fin])
    err = np.abs(g[fin] - w[fin])
    print("%s: worst |sum - fsum| / bound = %.3g" % (what, np.max(err / np.where(bound[fin] > 0, bound[fin], 1.0), initial=0.0)))
    assert np.all(err <= bound[fin]), (what, err, bound[fin])


def run_general(n_in, nz, ncol, strict, plant):
    models, g, boxes = pool(n_in)
    ins, truth, _ = make_state(n_in, nz, ncol, seed=1000 * nz + ncol, plant=plant)
    preds = predictions(n_in, nz, ins, strict, models)
    want = [ref.model_rows(n_in, ins, truth, preds[m], boxes[m]) for m in range(len(models))]
    if nz * ncol >= 17:
        assert any(np.all(w[2] > 0) for w in want), "no model has all four (side, class) classes"
        assert want[E_MODEL][2][1, 1] == 0 and want[E_MODEL][2][1, 0] > 0            # the n = 0 path
    tin, ttr = to_gpu(ins), to_gpu(truth)
    for k in (1, g, g + 1, 2 * g + 1):
        bank = bank_of(n_in, range(k))
        assert bank.domain_group == g and bank.models == k
        bank.set_domain(boxes[:k])
        bank.strict = int(strict)
        got, cnt = bank.evaluate_domain(nz, tin, ttr)
        whole, wcnt = bank.evaluate(nz, tin, ttr)
        bank.strict = 0
        assert got.shape == (k, 2, 2, 2, 4, 4) and cnt.shape == (k, 2, 2) and cnt.dtype == np.int64
        for m in range(k):
            check_model(got[m], cnt[m], want[m], "n_in %d (%d, %d) K %d strict %d plant %s model %d" % (n_in, nz, ncol, k, strict, plant, m))
            # against mw_surrogate_eval of the same call: the sides partition its cells, and the larger maximum is its maximum
            assert np.array_equal(cnt[m, 0] + cnt[m, 1], wcnt)
            for kind, row in ((0, m), (1, k)):
                assert np.array_equal(np.maximum(got[m, kind, 0, ..., 3], got[m, kind, 1, ..., 3]), whole[row, ..., 3], equal_nan=True)


CELLS5 = [1, 17, 33, 261, 70001]
SHAPES9 = [(1, 1), (2, 17), (9, 33), (17, 40)]
MULTI_CHUNK9 = [(9, 33), (17, 40)]


def chunk_of(nz, ncol):
    from miniweatherml_amd import capi
    return capi.lib().mw_mlp_stencil_chunk(nz, ncol)


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("ncells", CELLS5)
def test_single_cell_bank_against_the_reference(mw, ncells, strict):
    """n_in = 5, K in {1, g, g + 1, 2g + 1}, a different box per model: a lone cell, the tail of a tile, several tiles per wave, many blocks
    in the final pass; planted bounds, and (up to 261 cells) planted NaN and infinities in a second state."""
    run_general(5, 1, ncells, strict, "finite")
    if ncells <= 261:
        run_general(5, 1, ncells, strict, "nonfinite")


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", SHAPES9)
def test_stencil_bank_against_the_reference(mw, shape, strict):
    """n_in = 9: a level that is its own level above, column tails, more than one z chunk (asserted through mw_mlp_stencil_chunk)."""
    nz, ncol = shape
    if shape in MULTI_CHUNK9:
        assert chunk_of(nz, ncol) < nz, (shape, chunk_of(nz, ncol))
    run_general(9, nz, ncol, strict, "finite")
    run_general(9, nz, ncol, strict, "nonfinite")


@pytest.mark.parametrize("n_in", [5, 9])
def test_planted_values_follow_the_rule(mw, n_in):
    """The planted cells one by one, for model 0 alone: at lo and at hi inside, one nextafter beyond outside, NaN and the infinities outside
    its finite bounds; for model 2, +inf in density_dry inside its infinite bound; -0.0 inside lo = 0.0 of model 1 -- at level 0 (n_in = 5)
    and at the top level, which is its own level above.  The GPU's counts equal the reference's, whose mask is asserted here."""
    models, g, boxes = pool(n_in)
    nz, ncol = 3, 40
    ins, truth, planted = make_state(n_in, nz, ncol, seed=4, plant="nonfinite")
    assert len({(k, c) for k, c, _, _ in planted}) == len(planted)           # no plant overwrote another
    masks = [ref.outside_mask(n_in, ins, boxes[m]) for m in range(3)]
    b0 = boxes[0]
    for k, c, f, x in planted:
        if n_in == 9 and k != nz - 1:
            continue                                                         # (level 0 of a stencil model also answers for level 1)
        if f in (0, 1, 2):
            assert masks[0][k, c] == (not (f != 1 and (x == b0[f, 0] or x == b0[f, 1]))), (k, c, f, x)
        if f == 1 and x == INF:
            assert not ref.outside_mask(5, [a[k:k + 1, c:c + 1] for a in ins], np.where(np.arange(5)[:, None] == 1, boxes[2][1], OPEN[0]))
        if f in (3, 4):
            assert not ref.outside_mask(5, [a[k:k + 1, c:c + 1] for a in ins], np.where(np.arange(5)[:, None] == f, boxes[1][f], OPEN[0]))
    tin, ttr = to_gpu(ins), to_gpu(truth)
    bank = bank_of(n_in, range(3))
    bank.set_domain(boxes[:3])
    for strict in (0, 1):
        bank.strict = strict
        _, cnt = bank.evaluate_domain(nz, tin, ttr)
        bank.strict = 0
        act = ref.active_mask(ins, truth)
        for m in range(3):
            want = [[np.count_nonzero(~masks[m] & ~act), np.count_nonzero(~masks[m] & act)], [np.count_nonzero(masks[m] & ~act), np.count_nonzero(masks[m] & act)]]
            assert cnt[m].tolist() == want, (strict, m)
    # one bound moved by one ulp moves exactly the planted cells at it
    moved = boxes[:1].copy()
    moved[0, 0, 1] = np.nextafter(b0[0, 1], INF)                             # temp's hi: the cells one nextafter beyond are now inside
    bank1 = bank_of(n_in, [0])
    bank1.set_domain(boxes[:1])
    _, c_before = bank1.evaluate_domain(nz, tin, ttr)
    bank1.set_domain(moved)
    _, c_after = bank1.evaluate_domain(nz, tin, ttr)
    gain = int(np.count_nonzero(ref.outside_mask(n_in, ins, boxes[0]) & ~ref.outside_mask(n_in, ins, moved[0])))
    assert gain >= 1 and c_after[0, 0].sum() - c_before[0, 0].sum() == gain


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", MULTI_CHUNK9)
def test_stencil_level_above_across_a_chunk_edge(mw, shape, strict):
    """Width 9, every cell at the centre of the box but two: temp beyond hi at the FIRST level of the second z chunk (column c1) and at
    the top level (column c2).  Outside are exactly these two cells and the cells below them -- the one below the first is the last level
    of the chunk beneath and sees the value only as its level above; the top cell is its own level above.  The other columns stay inside.
    A bank of width 5 on the same state has the two cells alone."""
    nz, ncol = shape
    zc = chunk_of(nz, ncol)
    assert 1 <= zc < nz - 2
    c1, c2 = 3, ncol - 2
    for n_in in (9, 5):
        models, g, boxes = pool(n_in)
        box = boxes[0]
        rng = np.random.default_rng(nz)
        ins = [np.full((nz, ncol), 0.5 * (box[f, 0] + box[f, 1])) * (1.0 + 1e-3 * rng.random((nz, ncol))) for f in range(5)]
        ins[0][zc, c1] = np.nextafter(box[0, 1], INF)
        ins[0][nz - 1, c2] = np.nextafter(box[0, 1], INF)
        act = rng.random((nz, ncol)) < 0.5
        truth = [np.where(act, ins[i] * (1.0 + 1e-4), ins[i]) for i in BEFORE]
        mask = ref.outside_mask(n_in, ins, box)
        expect = np.zeros((nz, ncol), bool)
        expect[zc, c1] = expect[nz - 1, c2] = True
        if n_in == 9:
            expect[zc - 1, c1] = expect[nz - 2, c2] = True
        assert np.array_equal(mask, expect)
        bank = bank_of(n_in, [0])
        bank.set_domain(boxes[:1])
        bank.strict = strict
        got, cnt = bank.evaluate_domain(nz, to_gpu(ins), to_gpu(truth))
        bank.strict = 0
        assert cnt[0, 1].sum() == expect.sum() == (4 if n_in == 9 else 2)
        pred = predictions(n_in, nz, ins, strict, models[:1])[0]
        check_model(got[0], cnt[0], ref.model_rows(n_in, ins, truth, pred, box), "chunk edge n_in %d %r strict %d" % (n_in, shape, strict))


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in,shape", [(5, (1, 261)), (9, (9, 33))])
def test_mixed_state_and_tendency_bank(mw, n_in, shape, strict):
    """A bank that mixes both forms (the ANYT instantiations), more models than one pass holds."""
    models, g, boxes = pool(n_in)
    nz, ncol = shape
    k = g + 1
    forms = ["tendency" if m % 2 else "state" for m in range(k)]
    ins, truth, _ = make_state(n_in, nz, ncol, seed=31, plant="finite")
    preds = predictions(n_in, nz, ins, strict, models[:k], forms)
    bank = bank_of(n_in, range(k), forms)
    assert bank.forms == forms
    bank.set_domain(boxes[:k])
    bank.strict = strict
    got, cnt = bank.evaluate_domain(nz, to_gpu(ins), to_gpu(truth))
    bank.strict = 0
    for m in range(k):
        check_model(got[m], cnt[m], ref.model_rows(n_in, ins, truth, preds[m], boxes[m]), "mixed n_in %d strict %d model %d (%s)" % (n_in, strict, m, forms[m]))


EXACT_SHAPES = [(5, (1, 33)), (5, (1, 70001)), (9, (1, 1)), (9, (17, 40))]


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in,shape", EXACT_SHAPES)
@pytest.mark.parametrize("side", [0, 1])
def test_one_sided_boxes_give_the_parents_bytes(mw, n_in, shape, strict, side):
    """side 0: unbounded boxes -- every model's inside rows are mw_surrogate_eval's row of that model BIT FOR BIT, its persistence inside
    rows that call's persistence row, every outside number +0.0, the inside counts that call's counts and the outside counts 0.
    side 1: a box no cell satisfies (temp in [-1, -1]) -- the same with the sides exchanged."""
    models, g, _ = pool(n_in)
    nz, ncol = shape
    k = 2 * g + 1
    ins, truth, _ = make_state(n_in, nz, ncol, seed=7 + ncol, plant=None)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    box = OPEN.copy()
    if side == 1:
        box[0] = (-1.0, -1.0)
    bank = bank_of(n_in, range(k))
    bank.set_domain(np.stack([box] * k))
    bank.strict = strict
    got, cnt = bank.evaluate_domain(nz, tin, ttr)
    whole, wcnt = bank.evaluate(nz, tin, ttr)
    bank.strict = 0
    zeros = np.zeros((2, 4, 4)).tobytes()                                    # +0.0: the sign bit too
    for m in range(k):
        assert got[m, 0, side].tobytes() == whole[m].tobytes(), (m, "prediction")
        assert got[m, 1, side].tobytes() == whole[k].tobytes(), (m, "persistence")
        assert got[m, 0, 1 - side].tobytes() == zeros and got[m, 1, 1 - side].tobytes() == zeros, m
        assert np.array_equal(cnt[m, side], wcnt) and np.all(cnt[m, 1 - side] == 0), m
    assert wcnt.sum() == nz * ncol and (nz * ncol < 17 or np.all(wcnt > 0))


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in,shape", [(5, (1, 70001)), (9, (17, 40))])
def test_rows_do_not_depend_on_the_bank(mw, n_in, shape, strict):
    """A model's rows and counts are the same bytes alone, last of a bank of 2g + 1, and with the other models' boxes changed."""
    models, g, boxes = pool(n_in)
    nz, ncol = shape
    ins, truth, _ = make_state(n_in, nz, ncol, seed=77, plant="finite")
    tin, ttr = to_gpu(ins), to_gpu(truth)
    target = 2

    def run(idx, bx):
        bank = bank_of(n_in, idx)
        bank.set_domain(bx)
        bank.strict = strict
        out = bank.evaluate_domain(nz, tin, ttr)
        bank.strict = 0
        return out
    alone, acnt = run([target], boxes[[target]])
    assert acnt[0, 0].sum() > 0 and acnt[0, 1].sum() > 0
    others = [i for i in range(2 * g + 1) if i != target]
    idx = others + [target]
    got, cnt = run(idx, boxes[idx])
    assert got[-1].tobytes() == alone[0].tobytes() and cnt[-1].tobytes() == acnt[0].tobytes()
    changed = boxes[idx].copy()
    changed[:-1] = OPEN
    changed[0, 0] = (-1.0, -1.0)
    got2, cnt2 = run(idx, changed)
    assert got2[-1].tobytes() == alone[0].tobytes() and cnt2[-1].tobytes() == acnt[0].tobytes()
    assert got2[1].tobytes() != got[1].tobytes()                              # (the neighbours' rows did follow their boxes)
    # first of the bank, and on both sides of a pass boundary
    for pos in (0, g - 1, g):
        idx = others[:pos] + [target] + others[pos:]
        got, cnt = run(idx, boxes[idx])
        assert got[pos].tobytes() == alone[0].tobytes() and cnt[pos].tobytes() == acnt[0].tobytes(), pos


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in", [5, 9])
def test_poisoned_outside_cells_stay_outside(mw, n_in, strict):
    """A model whose prediction is NaN on outside cells only: density_dry is NaN on a few cells of either class (NaN is outside any box),
    which makes the predicted temp NaN there and nowhere else.  The outside rows of temp hold NaN sums and a NaN maximum in both classes;
    every inside row and every persistence row is finite (density_dry is no output)."""
    models, g, boxes = pool(n_in)
    nz, ncol = 5, 37
    ins, truth, _ = make_state(n_in, nz, ncol, seed=12, plant=None)
    act = ref.active_mask(ins, truth)
    cells = [tuple(c) for c in np.argwhere(act)[:3]] + [tuple(c) for c in np.argwhere(~act)[:3]]
    for k, c in cells:
        ins[1][k, c] = np.nan
    k = g + 1
    bx = np.stack([OPEN] * k)
    bank = bank_of(n_in, range(k))
    bank.set_domain(bx)
    bank.strict = strict
    got, cnt = bank.evaluate_domain(nz, to_gpu(ins), to_gpu(truth))
    bank.strict = 0
    for m in range(k):
        assert cnt[m].tolist() == [[int((~act).sum()) - 3, int(act.sum()) - 3], [3, 3]]
        assert np.all(np.isnan(got[m, 0, 1, :, 0, :])), (m, got[m, 0, 1, :, 0, :])
        assert np.all(np.isfinite(got[m, 0, 0])) and np.all(np.isfinite(got[m, 1])), m
        assert np.all(got[m, 0, 0, :, :, 1] > 0.0)


@pytest.mark.parametrize("n_in", [5, 9])
def test_nothing_is_written_to_the_fields(mw, n_in):
    models, g, boxes = pool(n_in)
    nz, ncol = 9, 33
    ins, truth, _ = make_state(n_in, nz, ncol, seed=5, plant="nonfinite")
    tin, ttr = to_gpu(ins), to_gpu(truth)
    bank = bank_of(n_in, range(g + 1))
    bank.set_domain(boxes[:g + 1])
    for strict in (0, 1):
        bank.strict = strict
        bank.evaluate_domain(nz, tin, ttr)
        bank.strict = 0
    for t, a in zip(tin + ttr, ins + truth):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_refusals_leave_the_outputs_alone(mw):
    """Every refusal of mw_surrogate_eval_domain -- the call before set_domain among them -- launches nothing: sentinel-filled out and counts
    stay as they were.  set_domain refuses lo > hi and NaN by name, and keeps the boxes it had."""
    import torch
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd._ffi import _field_ptr_array
    L = capi.lib()
    models, g, boxes = pool(5)
    bank = modules.SurrogateBank(models[:2])                                 # a fresh bank: no boxes yet
    nz, ncol = 2, 19
    ins, truth, _ = make_state(5, nz, ncol, seed=1, plant=None)
    tin, ttr = to_gpu(ins), to_gpu(truth)
    out = torch.full((2 * 128,), -7.25, dtype=torch.float64, device="cuda")
    cnt = torch.full((2 * 4,), -7, dtype=torch.int64, device="cuda")
    fin, ftr = _field_ptr_array(tin), _field_ptr_array(ttr)
    holed = _field_ptr_array(tin)
    holed[3] = None
    po, pc = C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())

    def refused(text, *args):
        assert L.mw_surrogate_eval_domain(*args) != 0
        assert text in L.mw_last_error(), L.mw_last_error()
        torch.cuda.synchronize()
        assert bool((out == -7.25).all()) and bool((cnt == -7).all()), text
    refused(b"no boxes", bank._h, nz, ncol, fin, ftr, po, pc, None)
    with pytest.raises(capi.MWError, match="no boxes"):
        bank.evaluate_domain(nz, tin, ttr)
    bank.set_domain(boxes[:2])
    refused(b"null pointer", None, nz, ncol, fin, ftr, po, pc, None)
    refused(b"null pointer", bank._h, nz, ncol, None, ftr, po, pc, None)
    refused(b"null pointer", bank._h, nz, ncol, fin, None, po, pc, None)
    refused(b"null pointer", bank._h, nz, ncol, fin, ftr, None, pc, None)
    refused(b"null pointer", bank._h, nz, ncol, fin, ftr, po, None, None)
    refused(b"nz and ncol", bank._h, 0, ncol, fin, ftr, po, pc, None)
    refused(b"nz and ncol", bank._h, nz, 0, fin, ftr, po, pc, None)
    refused(b"null field", bank._h, nz, ncol, holed, ftr, po, pc, None)
    refused(b"null field", bank._h, nz, ncol, fin, holed, po, pc, None)
    good, gcnt = bank.evaluate_domain(nz, tin, ttr)
    bad = boxes[:2].copy()
    bad[1, 2] = (1.0, 0.5)
    with pytest.raises(capi.MWError, match="box of model 1, field 2, is not lo <= hi"):
        bank.set_domain(bad)
    bad[1, 2] = (np.nan, 0.5)
    with pytest.raises(capi.MWError, match="box of model 1, field 2, is not lo <= hi .NaN is refused"):
        bank.set_domain(bad)
    with pytest.raises(capi.MWError, match=r"one \(5, 2\) box per model"):
        bank.set_domain(boxes[:3])
    again, acnt = bank.evaluate_domain(nz, tin, ttr)
    assert again.tobytes() == good.tobytes() and acnt.tobytes() == gcnt.tobytes() and np.array_equal(bank.boxes, boxes[:2])


# ---- evaluator class and driver -----------------------------------------------------------------------------------------------------
def write_models(tmp_path):
    """Two models, one of each width, as files: (entries of a surrogate_models list, the loaded tuples)."""
    from miniweatherml_amd import modules, surrogate_train as st
    entries = []
    for name, n_in, k in (("single_a", 5, 0), ("stencil_a", 9, 1)):
        net = pool(n_in)[0][k]
        paths = st.write_outputs(str(tmp_path / name), np.concatenate([np.ravel(a) for a in net[:4]]), net[4], net[5], {})
        entries.append({"name": name, "keras_weights_txt": paths[0], "nn_input_scaling": paths[1], "nn_output_scaling": paths[2]})
    return entries, modules.load_surrogate_bank(entries)


def same_result(a, b):
    return all(np.array_equal(x["sums"], y["sums"]) and np.array_equal(x["max"], y["max"]) and np.array_equal(x["counts"], y["counts"])
               and np.array_equal(x["nonfinite"], y["nonfinite"]) and x["calls"] == y["calls"] for x, y in zip(a, b)) and len(a) == len(b)


def test_evaluator_accumulates_what_combine_gives(mw, tmp_path):
    """Two accumulate calls on different states equal combine of the two single-call results with integer equality; the report's counts
    partition the cells and its inside + outside sums of squares are SurrogateEvaluator's."""
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    entries, nets = write_models(tmp_path)
    banks = [modules.SurrogateBank([nets[0]]), modules.SurrogateBank([nets[1]])]
    box = modules.domain_box([nets[0]], 0.0)
    ev = modules.DomainSplitEvaluator(banks, ["single_a", "stencil_a"], [box, box])
    plain = modules.SurrogateEvaluator(banks, ["single_a", "stencil_a"])
    coupler, dycore, micro = modules.make_supercell(16, 12, 10, 1, 8000., 6000., 20000.)
    singles = []
    for step in range(2):
        dt = dycore.compute_time_step(coupler)
        dycore.time_step(coupler, dt)
        coupler.get_data_manager_readwrite().get("cloud_liquid").add_(1e-4 * (step + 1))           # something for Kessler to do
        inp = Coupler("cuda:0")
        coupler.clone_into(inp)
        micro.time_step(coupler, dt)
        singles.append(ev.accumulate(inp, coupler))
        plain.accumulate(inp, coupler)
    assert same_result(ev.total, ev.combine(singles[0], singles[1])) and same_result(ev.total, ev.combine(singles[1], singles[0]))
    n = 16 * 12 * 10
    for ib in range(2):
        t = ev.total[ib]
        assert t["calls"] == 2 and t["sums"].dtype == object and int(t["counts"].sum()) == 2 * n and t["counts"][0, :, 1].sum() > 0
        # exact integers: inside + outside is the whole, up to the two roundings the device made (so: compare the counts exactly instead)
        assert np.array_equal(t["counts"][0].sum(axis=0), plain.total[ib]["counts"])
    rep = ev.report()
    assert set(rep) == {"single_a", "stencil_a"} and len(ev.history) == 2
    for name in rep:
        assert rep[name]["box"] == modules.box_json(box)
        assert rep[name]["inside"]["all"]["n"] + rep[name]["outside"]["all"]["n"] == 2 * n
        assert set(rep[name]["outside_share_of_squared_error"]) == {"inactive", "active", "all"}
    assert "stencil_a" in ev.table() and "share" in ev.table()
    json.dumps(ev.history, allow_nan=False)


def no_key(doc, key):
    if isinstance(doc, dict):
        return key not in doc and all(no_key(v, key) for v in doc.values())
    if isinstance(doc, list):
        return all(no_key(v, key) for v in doc)
    return True


def test_driver_eval_domain(mw, tmp_path, monkeypatch):
    """driver.run("evaluate_surrogates") on a 16 x 12 x 10 supercell with two models: with `eval_domain: {box_of: <first>}` the document has
    the domain block, one history entry per scoring step, counts that sum to the cells per model, and one box for both models; the final
    state is bitwise that of the run without the key, whose document has no `domain` key anywhere and is otherwise the same."""
    from test_gpu_driver import write_yaml
    from miniweatherml_amd import driver, modules
    entries, nets = write_models(tmp_path)
    models = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    docs, states = [], []
    for sub, key in (("with", "eval_domain: {box_of: single_a, margin: 0.0}\n"), ("without", "")):
        d = tmp_path / sub
        d.mkdir()
        path, _ = write_yaml(d, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=models + key)
        monkeypatch.chdir(d)
        coupler, _, info = driver.run("evaluate_surrogates", path, max_steps=2, quiet=True)
        docs.append(json.load(open(os.path.join(str(d), "surrogate_evaluation.json"))))
        dm = coupler.get_data_manager_readonly()
        states.append({n: dm.get(n, True).cpu().numpy().tobytes() for n in modules.ROLLOUT_FIELDS})
    doc, plain = docs
    assert states[0] == states[1]
    assert no_key(plain, "domain") and "domain" in doc
    assert {k: v for k, v in doc.items() if k not in ("domain", "yaml")} == {k: v for k, v in plain.items() if k != "yaml"}
    dom = doc["domain"]
    assert set(dom) == {"margin", "fields", "box_of", "group", "models", "history"}
    assert dom["margin"] == 0.0 and dom["fields"] == list(ref.IN5) and dom["box_of"] == "single_a"
    assert dom["group"] == {"5": pool(5)[1], "9": pool(9)[1]}
    assert list(dom["models"]) == ["single_a", "stencil_a"]
    box = modules.box_json(modules.domain_box([nets[0]], 0.0))
    assert dom["models"]["single_a"]["box"] == box and dom["models"]["stencil_a"]["box"] == box
    assert [h["step"] for h in dom["history"]] == [h["step"] for h in doc["history"]] == [0, 1]
    n = 16 * 12 * 10
    for h in dom["history"]:
        assert len(h["banks"]) == 2
        for b in h["banks"]:
            assert np.shape(b["stats"]) == (1, 2, 2, 2, 4, 4) and np.shape(b["counts"]) == (1, 2, 2) and int(np.sum(b["counts"])) == n
    for name in ("single_a", "stencil_a"):
        r = dom["models"][name]["report"]
        assert r["inside"]["all"]["n"] + r["outside"]["all"]["n"] == 2 * n and r["box"] == box
