"""The tendency form of the surrogate on the MI355X: the network predicts the change of the four fields and the kernels
add it in fp64 to the cell's own values.  Strict kernels against the numpy restatement (tests/tendency_ref.py) bit for bit; the MFMA
kernels by an exact identity (tendency = base + what the state-form kernel stores, where nothing is clipped), at the clip, and against the
strict form within the state-form comparison's tolerance; persistence bit for bit; the bank's promises (members_apply, eval, committee)
with both forms in one bank; the prepare kernel's labels; the trainer end to end; the rollout and inference drivers.

"Equal" is equality of the int64 views of the fp64 arrays throughout: the same bits."""
import ctypes
import json
import os

import numpy as np
import pytest

import tendency_ref as tr

pytestmark = pytest.mark.gpu

IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
OUT4 = ("temp", "water_vapor", "cloud_liquid", "precip_liquid")
STENCIL_NZ = (1, 2, 3, 22)                  # 22: three z chunks of the forward kernel at these column counts (asserted)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def gpu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def gpu_offset(a):
    """The same values in a view that starts one double into its allocation: 8 mod 16 bytes, so the 16-byte kernel is not taken."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


def run(fields, net, form, strict, nz=None, put=gpu):
    """mlp_forward / mlp_stencil_forward (nz given) of one form on host fields: four flat host arrays."""
    from miniweatherml_amd import modules
    t = [put(a) for a in fields]
    outs = [put(np.full(fields[0].shape, -7.0)) for _ in range(4)]
    if nz is None:
        modules.mlp_forward(*t, *net[:6], outs=outs, strict=strict, form=form)
    else:
        modules.mlp_stencil_forward(nz, *[x.view(nz, -1) for x in t], *net[:6], outs=[o.view(nz, -1) for o in outs], strict=strict, form=form)
    return [o.cpu().numpy().reshape(-1) for o in outs]


def shapes(n_in):
    """(shape, nz) of every case of one width: the single-cell sizes, or the stencil's levels x columns."""
    if n_in == 5:
        return [((n,), None) for n in tr.NCELLS]
    return [((nz, ncol), nz) for nz in STENCIL_NZ for ncol in tr.STENCIL_NCOL]


def test_the_stencil_shapes_cover_one_and_several_chunks(mw):
    from miniweatherml_amd import capi
    for ncol in tr.STENCIL_NCOL:
        assert all(capi.lib().mw_mlp_stencil_chunk(nz, ncol) == nz for nz in (1, 2, 3))
        zc = capi.lib().mw_mlp_stencil_chunk(22, ncol)
        assert zc < 22 and 22 % zc != 0, zc                                    # several chunks, the last one shorter


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. strict = the restatement
@pytest.mark.parametrize("n_in", [5, 9])
def test_strict_form_is_the_restatement_bit_for_bit(mw, n_in):
    net = tr.seeded_net(n_in, 11)
    for shape, nz in shapes(n_in):
        f = tr.inputs(shape, 21)
        want = tr.forward(f, net, "tendency", nz)
        got = run(f, net, "tendency", 1, nz)
        for j in range(4):
            assert same(got[j], want[j]), (shape, OUT4[j], np.max(np.abs(got[j] - want[j])))
        for j, (g, w) in enumerate(zip(run(f, net, "state", 1, nz), tr.forward(f, net, "state", nz))):      # form 0 through the same entry
            assert same(g, w), (shape, OUT4[j], "state")
    f = tr.inputs(shapes(n_in)[-1][0], 22)
    d = tr.change(f, net, shapes(n_in)[-1][1])
    assert (d > 0).any() and (d < 0).any()                                     # changes of both signs: the form is not a state model in disguise


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. MFMA: an identity without a tolerance
@pytest.mark.parametrize("n_in,put", [(5, gpu), (5, gpu_offset), (9, gpu)], ids=["single-16B", "single-offset", "stencil"])
def test_mfma_tendency_is_base_plus_the_state_kernels_output(mw, n_in, put):
    """Weight set P: d > 0 in every water cell, so the state-form kernel clips nothing and stores d itself; the tendency kernel of the same
    tables must then store base + d, one fp64 addition, in all four fields.  16-byte aligned arrays: k_mlp_x2 and its k_mlp remainder;
    views offset by one double: k_mlp alone; the stencil shapes: k_mlp_stencil."""
    net = tr.set_p(n_in)
    for shape, nz in shapes(n_in):
        f = tr.inputs(shape, 31)
        d_ref = tr.change(f, net, nz)
        assert np.count_nonzero(d_ref[1:] > 0) == d_ref[1:].size               # the share is 1: a condition on the inputs, checked on the CPU
        state, tend = run(f, net, "state", 0, nz, put), run(f, net, "tendency", 0, nz, put)
        for j in range(4):
            assert j == 0 or state[j].min() > 0
            assert same(tend[j], f[tr.BASE[j]].reshape(-1) + state[j]), (shape, OUT4[j])


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the clip
@pytest.mark.parametrize("n_in,shape,nz", [(5, (2113,), None), (9, (22, 33), 22)])
def test_clamp_at_zero(mw, n_in, shape, nz):
    """Weight set N with water drawn around -d: base + d < 0 in about half of the water cells.  Where the restatement is below zero by more
    than the tolerance the MFMA kernel stores exactly +0.0; everywhere else it agrees with the strict kernel within the tolerance."""
    net = tr.set_n(n_in)
    f = tr.inputs_for_clamp(shape, 41, net, nz)
    raw = [f[tr.BASE[j]].reshape(-1) + tr.change(f, net, nz)[j] for j in range(4)]
    tol = tr.tol(net[5])
    strict, fast = run(f, net, "tendency", 1, nz), run(f, net, "tendency", 0, nz)
    for j in (1, 2, 3):
        share = float(np.mean(raw[j] < 0))
        print("%s: base + d < 0 in %.3f of the cells" % (OUT4[j], share))
        assert 0.25 <= share <= 0.75, (OUT4[j], share)
        clear = raw[j] < -tol[j]
        assert clear.any() and np.all(bits(fast[j][clear]) == 0), OUT4[j]      # +0.0, not -0.0, not a small number
        assert np.all(bits(strict[j][raw[j] < 0]) == 0)
        assert fast[j].min() >= 0.0 and np.max(np.abs(fast[j][~clear] - strict[j][~clear])) <= tol[j], OUT4[j]
    assert np.max(np.abs(fast[0] - strict[0])) <= tol[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. MFMA against strict
@pytest.mark.parametrize("n_in", [5, 9])
def test_mfma_form_against_the_strict_form(mw, n_in):
    """|y_mfma - y_strict| <= 1e-5 (|out_min| + out_rng) per field: the state-form comparison's relative tolerance on the scale of d."""
    worst = np.zeros(4)
    for seed in (11, 12):
        net = tr.seeded_net(n_in, seed)
        tol = tr.tol(net[5])
        for shape, nz in shapes(n_in):
            f = tr.inputs(shape, 51 + seed)
            strict, fast = run(f, net, "tendency", 1, nz), run(f, net, "tendency", 0, nz)
            for j in range(4):
                worst[j] = max(worst[j], np.max(np.abs(fast[j] - strict[j])) / tol[j])
    print("n_in %d: largest |mfma - strict| in units of the bound, per field: %s" % (n_in, np.array2string(worst, precision=3)))
    assert np.all(worst <= 1.0), worst


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. persistence
@pytest.mark.parametrize("n_in", [5, 9])
def test_a_zero_change_returns_the_input_bit_for_bit(mw, n_in):
    """W2 = 0, b2 = 0, out_min = 0 through the MFMA and the strict kernels (aligned, offset, every shape) and through members_apply in place:
    every output is its input field, bit for bit -- exact zeros and values down to 1e-30 included."""
    import torch
    from miniweatherml_amd import modules
    net = tr.persistence_net(n_in)
    for shape, nz in shapes(n_in):
        f = tr.inputs(shape, 61)
        for strict in (0, 1):
            for put in ((gpu, gpu_offset) if n_in == 5 else (gpu,)):
                got = run(f, net, "tendency", strict, nz, put)
                for j in range(4):
                    assert same(got[j], f[tr.BASE[j]].reshape(-1)), (shape, strict, OUT4[j])
    bank = modules.SurrogateBank([net + ("tendency",), tr.persistence_net(n_in, 1) + ("tendency",)])
    for nz, ncol in ((3, 17), (22, 33)):
        f = tr.inputs((nz, ncol, 3), 62)
        for strict in (0, 1):
            t = [gpu(a) for a in f]
            bank.strict = strict
            bank.members_apply(nz, [2, 0], t)
            torch.cuda.synchronize()
            for i in range(5):
                assert same(t[i].cpu().numpy(), f[i]), (nz, ncol, strict, IN5[i])


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the bank's promises with both forms in one bank
def bank_models(n_in):
    """state, tendency, and a tendency model with other scaling tables (inputs and outputs)."""
    a, b = tr.seeded_net(n_in, 71), tr.seeded_net(n_in, 72)
    c = tr.seeded_net(n_in, 73, scale_out=((-2.0, -1e-3, -2e-3, -1e-3), (5.0, 4e-3, 1e-3, 3e-3)))
    c = c[:4] + (np.ascontiguousarray(c[4] * np.array([[0.95, 1.04]]) + np.array([[0.0, 1e-4]])), c[5])
    return [a + ("state",), b + ("tendency",), c + ("tendency",)]


_BANKS = {}


def bank_of(n_in, idx):
    from miniweatherml_amd import modules
    key = (n_in, tuple(idx))
    if key not in _BANKS:
        _BANKS[key] = modules.SurrogateBank([bank_models(n_in)[i] for i in idx])
    return _BANKS[key]


def forwards(n_in, f, strict):
    """[model][field] host arrays (nz, ncol) from the _form forward kernels on contiguous fields."""
    nz = f[0].shape[0]
    return [[o.reshape(f[0].shape) for o in run(f, m, m[6], strict, nz if n_in == 9 else None)] for m in bank_models(n_in)]


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in", [5, 9])
def test_members_apply_writes_the_forward_kernels_bits(mw, n_in, strict):
    import torch
    from miniweatherml_amd import capi
    assert bank_of(n_in, (0, 1, 2)).forms == ["state", "tendency", "tendency"]
    assert [capi.lib().mw_surrogate_bank_form(bank_of(n_in, (0, 1, 2))._h, m) for m in (0, 1, 2, 3)] == [0, 1, 1, -1]
    for nz, ncol in ((1, 1), (3, 17), (22, 33), (2, 97)):
        f = tr.inputs((nz, ncol, 3), 81)
        for idx, members in (((0, 1, 2), [2, 0, 1]), ((2, 0), [2, 0])):       # the second: member 1 belongs to nobody
            t = [gpu(a) for a in f]
            bank = bank_of(n_in, idx)
            bank.strict = strict
            bank.members_apply(nz, members, t)
            torch.cuda.synchronize()
            bank.strict = 0
            now = [x.cpu().numpy() for x in t]
            assert same(now[1], f[1])                                          # density_dry
            for k, e in zip(idx, members):
                want = forwards(n_in, [np.ascontiguousarray(a[..., e]) for a in f], strict)[k]
                for j in range(4):
                    assert same(now[tr.BASE[j]][..., e], want[j]), (nz, ncol, idx, "model", k, "member", e, OUT4[j])
            for e in set(range(3)) - set(members):
                for i in range(5):
                    assert same(now[i][..., e], f[i][..., e]), (nz, ncol, "untouched member", e, IN5[i])


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in", [5, 9])
def test_eval_scores_each_models_own_form(mw, n_in, strict):
    """mw_surrogate_eval's rows against statistics computed on the host from each model's forward output; the rows do not depend on the
    other models of the bank or on a model's place in it."""
    from test_gpu_surrogate_eval import check_rows, host_stats
    for nz, ncol in ((3, 17), (22, 33)):
        f = tr.inputs((nz, ncol), 91)
        rng = np.random.default_rng(92)
        act = rng.random((nz, ncol)) < 0.5
        truth = [np.where(act, f[tr.BASE[j]] + rng.uniform(1e-3, 1e-2, (nz, ncol)) * s * rng.choice([-1.0, 1.0], (nz, ncol)), f[tr.BASE[j]])
                 for j, s in enumerate((5.0, 4e-3, 2e-3, 2e-3))]
        per_model = forwards(n_in, f, strict)
        rows = [host_stats(p, truth, f) for p in per_model] + [host_stats([f[i] for i in tr.BASE], truth, f)]
        tin, ttr = [gpu(a) for a in f], [gpu(a) for a in truth]
        got = {}
        for idx in ((0, 1, 2), (2, 0), (1,)):
            bank = bank_of(n_in, idx)
            bank.strict = strict
            got[idx], counts = bank.evaluate(nz, tin, ttr)
            bank.strict = 0
            check_rows(got[idx], counts, [rows[i] for i in idx] + rows[-1:], "n_in %d (%d, %d) bank %r strict %d" % (n_in, nz, ncol, idx, strict))
        assert same(got[(2, 0)][0], got[(0, 1, 2)][2]) and same(got[(2, 0)][1], got[(0, 1, 2)][0]) and same(got[(1,)][0], got[(0, 1, 2)][1])
        assert not same(got[(0, 1, 2)][1], got[(0, 1, 2)][0])


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in", [5, 9])
def test_committees_of_one_and_of_mixed_forms(mw, n_in, strict):
    """A committee of one tendency model returns that model's bits; a mixed committee of three is committee_ref.combine of the three forward
    outputs, range included; in place and out of place give the same bits, and the other members keep theirs."""
    import torch
    import committee_ref as R
    bank = bank_of(n_in, (0, 1, 2))
    for nz, ncol, nens, member in ((1, 1, 1, 0), (3, 17, 1, 0), (22, 33, 3, 1), (2, 97, 3, 2)):
        f = tr.inputs((nz, ncol, nens), 101)
        per_model = forwards(n_in, [np.ascontiguousarray(a[..., member]) for a in f], strict)
        bank.strict = strict
        for sel in ([1], [2], [2, 0, 1], [0, 1]):
            pairs = [R.combine([per_model[k][j] for k in sel]) for j in range(4)]
            t = [gpu(a) for a in f]
            outs, rngs = [torch.full_like(t[0], -7.0) for _ in range(4)], [torch.full_like(t[0], -7.0) for _ in range(4)]
            bank.committee_apply(nz, sel, member, t, outs, rngs)
            for j in range(4):
                assert R.same_bits(outs[j].cpu().numpy()[..., member], pairs[j][0]), (nz, ncol, sel, OUT4[j])
                assert R.same_bits(rngs[j].cpu().numpy()[..., member], pairs[j][1]), (nz, ncol, sel, OUT4[j], "range")
                if len(sel) == 1:
                    assert same(outs[j].cpu().numpy()[..., member], per_model[sel[0]][j])
            rin = [torch.full_like(t[0], -7.0) for _ in range(4)]
            bank.committee_apply(nz, sel, member, t, [t[i] for i in tr.BASE], rin)                 # in place
            for j in range(4):
                now = t[tr.BASE[j]].cpu().numpy()
                assert same(now[..., member], outs[j].cpu().numpy()[..., member]), (nz, ncol, sel, OUT4[j], "in place")
                assert same(rin[j].cpu().numpy(), rngs[j].cpu().numpy())
                others = [e for e in range(nens) if e != member]
                assert same(now[..., others], f[tr.BASE[j]][..., others])
            assert same(t[1].cpu().numpy(), f[1])
    bank.strict = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. the prepare kernel's labels
def device_prepare(form, n_in, raw_in, raw_out, si, so, seed, n_train, n_val):
    """mw_surrogate_prepare_form (form 0 | 1) or mw_surrogate_prepare_v2 (form None) on host arrays: the return code and the six arrays."""
    import torch
    from miniweatherml_amd import capi
    n = raw_in.shape[0]
    dev_in, dev_out = torch.from_numpy(np.ascontiguousarray(raw_in)).cuda(), torch.from_numpy(np.ascontiguousarray(raw_out)).cuda()
    sizes = [(rows, max(k, 0)) for k in (n_train, n_val, n - n_train - n_val) for rows in (n_in, 4)]
    outs = [torch.full((max(rows * k, 1),), float("nan"), dtype=torch.float32, device="cuda") for rows, k in sizes]
    dp, ptr = ctypes.POINTER(ctypes.c_double), lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    args = [n_in, n, ptr(dev_in), ptr(dev_out), si.ctypes.data_as(dp), so.ctypes.data_as(dp), seed, n_train, n_val] + [ptr(t) for t in outs] + [None]
    L = capi.lib()
    rc = L.mw_surrogate_prepare_v2(*args) if form is None else L.mw_surrogate_prepare_form(form, *args)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy()[:rows * k].reshape(rows, k) for t, (rows, k) in zip(outs, sizes)]


@pytest.mark.parametrize("n", [1, 3, 7, 1000])
@pytest.mark.parametrize("n_in", [5, 9])
def test_prepare_writes_the_label_expression(mw, n_in, n):
    """x sets: those of _v2, bit for bit.  y sets: (float)((((double)out - (double)in[base]) - min) / (max - min)) in numpy.  form 0: _v2 in
    every array.  One sample cannot fill three sets: both entry points refuse it with the same words (n = 3 is the smallest that runs)."""
    from surrogate_ref import raw_samples
    from miniweatherml_amd import capi, surrogate_train as st
    x, y = raw_samples(max(n, 3), n_in, n)
    y = (x[:, list(tr.BASE)] + (y - y.mean(0)) * np.float32(1e-2)).astype(np.float32)
    si, so = st.data_scaling(x, y, form="tendency")
    si0, so0 = st.data_scaling(x, y)
    x, y = x[:n], y[:n]
    if n < 3:
        msgs = []
        for form in (None, 0, 1):
            rc, _ = device_prepare(form, n_in, x, y, si, so, 5, 1, 0)
            msgs.append((rc != 0, capi.lib().mw_last_error()))
        assert msgs[0][0] and msgs[0] == msgs[1] == msgs[2] and b"every set needs at least one sample" in msgs[0][1]
        return
    n_train, n_val = (1, 1) if n == 3 else st.split_sizes(n)[:2]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)                            # noqa: E731
    rc_t, tend = device_prepare(1, n_in, x, y, si, so, 5, n_train, n_val)
    rc_v, v2 = device_prepare(None, n_in, x, y, si, so, 5, n_train, n_val)
    assert rc_t == 0 and rc_v == 0
    perm = st.preshuffle_permutation(n, 5)
    d = y.astype(np.float64)[perm] - x.astype(np.float64)[perm][:, list(tr.BASE)]
    lab = ((d - so[:, 0]) / (so[:, 1] - so[:, 0])).astype(np.float32)
    cut = [0, n_train, n_train + n_val, n]
    for k in range(3):
        assert np.array_equal(f32(tend[2 * k]), f32(v2[2 * k])), ("x", k)
        assert np.array_equal(f32(tend[2 * k + 1]), f32(lab[cut[k]:cut[k + 1]].T)), ("y", k)
    assert not np.array_equal(tend[1], v2[1])
    rc_0, zero = device_prepare(0, n_in, x, y, si0, so0, 5, n_train, n_val)
    rc_v, v2 = device_prepare(None, n_in, x, y, si0, so0, 5, n_train, n_val)
    assert rc_0 == 0 and rc_v == 0 and all(np.array_equal(f32(a), f32(b)) for a, b in zip(zero, v2))


# ---------------------------------------------------------------------------------------------------------------------------------
# 12. the trainer end to end
def smooth_samples(n, seed):
    """inputs (n, 5, 2) and outputs (n, 4) fp32: outputs = inputs + a small smooth function of them (condensation-like: vapor to cloud with
    warming, cloud to rain), the level above a shifted copy."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(tr.IN_LO[i], tr.IN_HI[i], n) for i in range(5)], axis=1)
    u = (x - tr.IN_LO) / (tr.IN_HI - tr.IN_LO)
    cond = 1e-3 * (u[:, 2] - 0.5) * u[:, 0]
    auto = 5e-4 * u[:, 3] ** 2
    y = np.stack([x[:, 0] + 2500.0 * cond, x[:, 2] - cond, x[:, 3] + cond - auto, x[:, 4] + auto], axis=1)
    return np.stack([x, np.roll(x, 1, axis=0)], axis=2).astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("stencil", [False, True])
def test_trainer_end_to_end(mw, tmp_path, stencil):
    import torch
    from test_surrogate_train_cpu import write_sample_file
    from miniweatherml_amd import modules, surrogate_train as st
    i3, o2 = smooth_samples(4000, 3)
    path = write_sample_file(tmp_path / "samples.nc", [(i3, o2)])
    out = str(tmp_path / "model")
    r = st.train_surrogate([path], out, epochs=3, batch_size=256, models=2, seed=4, stencil=stencil, form="tendency")
    assert r["form"] == "tendency" and json.load(open(os.path.join(out, "history.json")))["form"] == "tendency"
    for m, h in enumerate(r["history"]):
        print("model %d loss per epoch: %s" % (m, h["loss"]))
        assert h["loss"][2] < h["loss"][0], (m, h["loss"])
    model = modules.load_surrogate_model(*r["files_written"])
    assert model.form == "tendency" and model.W1.shape == ((9 if stencil else 5), 10)
    x, y, _ = st.read_samples([path], stencil=stencil)
    assert np.array_equal(model.scl_out, st.data_scaling(x, y, form="tendency")[1])
    # the written model through mlp_forward(form="tendency") against the Trainer's own prediction of the test set, un-scaled + base
    split = (r["n_train"], r["n_val"], r["n_test"])
    trn = st.Trainer(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), model.scl_in, model.scl_out, split, seed=4, models=1,
                     batch_size=256, epochs=1, form="tendency")
    o = trn.predict_test(r["weights"][r["best_model"]]).cpu().numpy()
    test = st.preshuffle_permutation(x.shape[0], 4)[split[0] + split[1]:]
    base = x.astype(np.float64)[test][:, list(tr.BASE)].T
    want = base + tr.unscaled(o, model.scl_out)
    want[1:] = np.maximum(0.0, want[1:])
    xt = x.astype(np.float64)[test]
    ins = [gpu(xt[:, i]) for i in range(5)]
    if stencil:      # two levels per sample: level 0 the cell, level 1 (the top: its own level above) built from features 5..8
        lev1 = [xt[:, 5], xt[:, 1], xt[:, 6], xt[:, 7], xt[:, 8]]
        ins = [gpu(np.stack([xt[:, i], lev1[i]])) for i in range(5)]
        got = [g.cpu().numpy()[0] for g in modules.mlp_stencil_forward(2, *ins, *model[:6], form="tendency")]
    else:
        got = [g.cpu().numpy() for g in modules.mlp_forward(*ins, *model[:6], form="tendency")]
    tol = tr.tol(model.scl_out)
    for j in range(4):
        err = np.max(np.abs(got[j] - want[j]))
        print("%s: max |forward - trainer's prediction| = %.3g = %.3g of the bound" % (OUT4[j], err, err / tol[j]))
        assert err <= tol[j], (OUT4[j], err / tol[j])
    # --init continues it: the form comes from the directory, and the first epoch starts where the run ended
    r2 = st.train_surrogate([path], str(tmp_path / "more"), epochs=1, batch_size=256, models=1, seed=9, stencil=stencil, init=out)
    assert r2["form"] == "tendency" and modules.load_surrogate_model(*r2["files_written"]).form == "tendency"
    assert np.array_equal(r2["output_scaling"], model.scl_out) and r2["history"][0]["loss"][0] < r["history"][r["best_model"]]["loss"][0]
    with pytest.raises(st.SurrogateTrainError, match="cannot be continued as a state-form"):
        st.train_surrogate([path], None, epochs=1, init=out, form="state")


# ---------------------------------------------------------------------------------------------------------------------------------
# 13. the drivers
def write_two_models(tmp_path):
    """A state and a tendency model of the single-cell width as files: the entries of a surrogate_models list."""
    from miniweatherml_amd import modules, surrogate_train as st
    entries = []
    shipped = modules.load_surrogate_weights()
    W1, b1, W2, b2, _, _ = tr.set_p(5, 5)                                      # o = 0.5 +- a little: small changes of both signs around 0
    so_t = np.ascontiguousarray([[-0.5, 0.5], [-1e-5, 1e-5], [-1e-5, 1e-5], [-1e-5, 1e-5]])
    for name, net, form in (("state_a", shipped, "state"), ("tend_a", (W1, b1, W2, b2, shipped[4], so_t), "tendency")):
        paths = st.write_outputs(str(tmp_path / name), np.concatenate([np.ravel(a) for a in net[:4]]), net[4], net[5], {}, form=form)
        entries.append({"name": name, "keras_weights_txt": paths[0], "nn_input_scaling": paths[1], "nn_output_scaling": paths[2]})
    return entries


def test_drivers_run_a_tendency_model(mw, tmp_path, monkeypatch, capsys):
    """rollout_surrogates with one state and one tendency model on the 16 x 12 x 10 grid of the existing rollout tests: the tendency
    member's fields equal a replay in which that member is overwritten each step by mlp_forward(form="tendency") of its own values before
    the step; the JSON names both forms.  inference_ponni on the tendency directory runs and says which form it ran."""
    import torch
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_rollout import ALL8, fields
    from miniweatherml_amd import driver, modules, rollout
    entries = write_two_models(tmp_path)
    extra = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in entries)
    path, _ = write_yaml(tmp_path, nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
    monkeypatch.chdir(tmp_path)
    coupler, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert doc["members"] == ["kessler", "state_a", "tend_a", "persistence"]
    assert [(m["name"], m["form"], m["member"]) for m in doc["models"]] == [("state_a", "state", 1), ("tend_a", "tendency", 2)]
    got = fields(coupler, ALL8)
    tend = modules.load_surrogate_model(entries[1]["keras_weights_txt"], entries[1]["nn_input_scaling"], entries[1]["nn_output_scaling"])
    assert tend.form == "tendency"

    class Replay(rollout.Microphysics_Rollout):
        def time_step(self, coupler, dt):
            dm = coupler.get_data_manager_readwrite()
            before = [dm.get(n)[..., 2].contiguous() for n in IN5]
            super().time_step(coupler, dt)
            outs = modules.mlp_forward(*before, *tend[:6], form="tendency")
            for n, o in zip(OUT4, outs):
                dm.get(n)[..., 2].copy_(o)

    state_twice = [entries[0], dict(entries[0], name="tend_a")]                # the replay's own member-2 model is a state model: overwritten
    extra2 = "surrogate_models:\n" + "".join("  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in e.items()) for e in state_twice)
    path2, _ = write_yaml(tmp_path, nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra2)
    monkeypatch.setattr(rollout, "Microphysics_Rollout", Replay)
    coupler2, _, _ = driver.run("rollout_surrogates", path2, max_steps=3, quiet=True)
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    want = fields(coupler2, ALL8)
    for n in ALL8:
        assert torch.equal(got[n][..., 2].contiguous().view(torch.int64), want[n][..., 2].contiguous().view(torch.int64)), n
        assert torch.equal(got[n][..., 1].contiguous().view(torch.int64), want[n][..., 1].contiguous().view(torch.int64)), n
    assert not torch.equal(got["temp"][..., 2], got["temp"][..., 3])           # the member moved away from persistence
    assert torch.isfinite(got["temp"]).all()
    # inference_ponni reads the form from the files
    e = entries[1]
    extra3 = "".join('%s: "%s"\n' % (k, e[k]) for k in ("keras_weights_txt", "nn_input_scaling", "nn_output_scaling"))
    path3, _ = write_yaml(tmp_path, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra3)
    capsys.readouterr()
    c3, _, info3 = driver.run("inference_ponni", path3, max_steps=2, quiet=False)
    out = capsys.readouterr().out
    assert info3["steps"] == 2 and info3["surrogate_form"] == "tendency" and "surrogate output form: tendency" in out
    assert len([ln for ln in out.splitlines() if ln.startswith("Relative diff")]) == 8
    # evaluate_surrogates names the forms too
    path4, _ = write_yaml(tmp_path, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
    driver.run("evaluate_surrogates", path4, max_steps=2, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_evaluation.json")))
    assert [(m["name"], m["form"]) for m in doc["models"]] == [("state_a", "state"), ("tend_a", "tendency")]
