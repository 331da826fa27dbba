"""The dense-stack forward kernels (csrc/mw_mlp_stack.hip) against two numpy statements of the network on the fp32 scaled
inputs: an fp64 forward of the fp32 weights, and the fp32 index-order loop (acc += x * w per product, then bias, then activation).

Yardstick of the production kernel, in scaled output space and per output field (the factor 4: DESIGN.md 13, the rho criterion of the
trainer's gradient; the floor covers shapes where the plain loop happens to be exact):
    max|o_kernel - o_fp64| <= 4 * max|o_fp32loop - o_fp64| + 2^-23 * max|o_fp64|
The right-hand side is a figure of the SHAPE: the plain loop's error for these weights over the cells of all calls of one (shape, form),
434 for n_in = 5.  The left-hand side is per call, and every call is held to it: one cell gives no error estimate of its own.  (Held to its
own cells' right-hand side, 3 of the 178 calls miss, at 1.33, 1.39, 1.46 of it: 5->[15] tendency 1 cell field 2, 2.877e-08 > 2.163e-08;
5->[17, 3, 64] tendency 15 cells field 3, 1.838e-07 > 1.324e-07; 5->[64] * 4 tendency 1 cell field 1, 2.150e-08 > 1.468e-08.)
o_kernel is recovered from the stored fp64 field, (y - base - min) / rng rounded to fp32; the un-scaling, base and clip are held to 2 ulp
of fp64 from it.  A clipped cell shows no output: there the fp64 reference must itself lie below the bound.

Measured on an MI355X, the worst left / right over a shape's calls, state | tendency:
    5->[1] .114 .141   5->[3] .190 .190   5->[4] .139 .139   5->[5] .178 .201   5->[15] .180 .180   5->[16] .208 .208   5->[17] .175 .177
    5->[33] .243 .304   5->[64] .424 .424   5->[17, 3, 64] .301 .573   5->[64] * 4 .302 .366   9->[10] .203 .203   9->[17, 5] .243 .252
Every width class, every pair of layer shapes and a second grid pass are held to the same yardstick in test_gpu_stack_shapes.py, whose
header has its ratios per depth.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, [1]), (5, [3]), (5, [4]), (5, [5]), (5, [15]), (5, [16]), (5, [17]), (5, [33]), (5, [64]), (5, [17, 3, 64]), (5, [64, 64, 64, 64]),
          (9, [10]), (9, [17, 5])]
NCELLS = (1, 15, 16, 17, 63, 65, 257)                      # 64 cells: the four tiles of one wave's iteration; 256: those of one workgroup
NZ_NCOL = [(nz, ncol) for nz in (1, 2, 3) for ncol in (1, 17)]
SLOPES = (0.1, 0.0, 1.0, 0.25)
BOX = [[220., 320.], [0.2, 1.3], [0., 0.02], [0., 0.004], [0., 0.008], [220., 320.], [0., 0.02], [0., 0.004], [0., 0.008]]


def make_stack(n_in, widths, form, seed):
    """Random weights of Keras' magnitude (glorot_uniform), slopes that walk through 0 and 1, output tables that reach below zero."""
    from miniweatherml_amd import mlp
    rng = np.random.default_rng(seed)
    w = [n_in] + list(widths) + [4]
    layers = [(rng.uniform(-1, 1, (a, b)).astype(np.float32) * np.float32(np.sqrt(6.0 / (a + b))), rng.uniform(-0.2, 0.2, b).astype(np.float32))
              for a, b in zip(w[:-1], w[1:])]
    scl_out = [[-4., 6.], [-2e-3, 3e-3], [-1e-3, 2e-3], [-2e-3, 2e-3]] if form == "tendency" else [[230., 310.], [-4e-3, 0.02], [-1e-3, 0.004], [-2e-3, 0.008]]
    return mlp.SurrogateStack(layers, np.array([SLOPES[(seed + l) % 4] for l in range(len(widths))], np.float32), np.array(BOX[:n_in]), np.array(scl_out), form)


def make_fields(ncells, seed):
    """The five fields spread over the scaling box and a tenth of its range beyond either side."""
    rng = np.random.default_rng(1000 + seed)
    return [lo + (1.2 * rng.random(ncells) - 0.1) * (hi - lo) for lo, hi in BOX[:5]]


def features(stack, fields, nz):
    from miniweatherml_amd import mlp
    return mlp.stencil_features(fields, nz).T if stack.scl_in.shape[0] == 9 else np.stack(fields, 1)


def references(stack, X):
    """(o_fp64, o_fp32loop), each (ncells, 4), from the inputs scaled in fp64 and stored as fp32."""
    a32 = ((X - stack.scl_in[:, 0]) / (stack.scl_in[:, 1] - stack.scl_in[:, 0])).astype(np.float32)
    a64 = a32.astype(np.float64)
    for l, (W, b) in enumerate(stack.layers):
        a64 = a64 @ W.astype(np.float64) + b
        acc = np.zeros((X.shape[0], W.shape[1]), np.float32)
        for i in range(W.shape[0]):
            acc += a32[:, i:i + 1] * W[i]
        a32 = acc + b
        if l < len(stack.layers) - 1:
            s = np.float32(stack.slopes[l])
            a64, a32 = np.where(a64 > 0, a64, float(s) * a64), np.where(a32 > 0, a32, s * a32)
    return a64, a32


def unscale(stack, o, X, clip=True):
    from miniweatherml_amd import mlp
    y = o.astype(np.float64) * (stack.scl_out[:, 1] - stack.scl_out[:, 0]) + stack.scl_out[:, 0]
    if stack.form == "tendency":
        y = X[:, list(mlp.BASE4)] + y
    if clip:
        y[:, 1:] = np.maximum(0.0, y[:, 1:])
    return y


def run(handle, fields, nz, strict=0, tail=0):
    """The kernel's four fields as (ncells, 4); tail: sentinel cells behind every array, which must come back untouched."""
    n = fields[0].size
    dev = [torch.full((n + tail,), -7.5, dtype=torch.float64, device="cuda") for _ in range(9)]
    for d, f in zip(dev, fields):
        d[:n] = torch.from_numpy(np.ascontiguousarray(f))
    y = handle.forward(nz, *[d[:n] for d in dev[:5]], outs=[d[:n] for d in dev[5:]], strict=strict)
    assert all(bool((d[n:] == -7.5).all()) for d in dev), "a cell behind an array was written"
    assert all(np.array_equal(d[:n].cpu().numpy().view(np.int64), f.view(np.int64)) for d, f in zip(dev[:5], fields)), "an input was written"
    return np.stack([t.cpu().numpy() for t in y], 1)


def shape_bound(stack, Xs):
    """The yardstick's right-hand side per output field, over the cells of every call in Xs."""
    refs = [references(stack, X) for X in Xs]
    return 4 * np.max([np.abs(o32 - o64).max(0) for o64, o32 in refs], 0) + 2.0 ** -23 * np.max([np.abs(o64).max(0) for o64, _ in refs], 0)


def held_to_yardstick(stack, X, y, what, bounds):
    """One call against the yardstick of this file's header, every figure printed: (the worst err / bound of its four fields, the misses)."""
    from miniweatherml_amd import mlp
    rng_o, min_o = stack.scl_out[:, 1] - stack.scl_out[:, 0], stack.scl_out[:, 0]
    o64 = references(stack, X)[0]
    base = X[:, list(mlp.BASE4)] if stack.form == "tendency" else 0.0
    live = np.ones(y.shape, bool)
    live[:, 1:] = y[:, 1:] > 0                                        # a clipped cell does not show the kernel's output
    ok = (((y - base) - min_o) / rng_o).astype(np.float32)            # the kernel's own fp32 output
    again = unscale(stack, ok, X)
    assert np.all(np.abs(again - y)[live] <= 2 * np.spacing(np.abs(y))[live]), what + ": un-scaling, base or clip"
    worst, misses = 0.0, []
    for n in range(4):
        m = live[:, n]
        bound = bounds[n]
        err = float(np.max(np.abs(ok - o64)[m, n])) if m.any() else 0.0
        print("%s field %d: err %.3e bound %.3e ratio %.3f clipped %d" % (what, n, err, bound, err / bound, (~m).sum()))
        if err > bound:
            misses.append("%s field %d: %.3e > %.3e" % (what, n, err, bound))
        assert np.all(unscale(stack, o64, X, clip=False)[~m, n] <= bound * rng_o[n]), what + ": a cell was clipped that the reference keeps"
        worst = max(worst, err / bound)
    return worst, misses


@pytest.mark.parametrize("form", ["state", "tendency"])
@pytest.mark.parametrize("ishape", range(len(SHAPES)))
def test_production_kernel_against_fp64(mw, ishape, form):
    from miniweatherml_amd import mlp
    n_in, widths = SHAPES[ishape]
    stack = make_stack(n_in, widths, form, ishape)
    handle = mlp.MlpStack(stack, "cuda")
    worst, clipped, misses = 0.0, 0, []
    calls = [(nz, make_fields(nz * ncol, ishape)) for nz, ncol in (NZ_NCOL if n_in == 9 else [(1, n) for n in NCELLS])]
    bounds = shape_bound(stack, [features(stack, fields, nz) for nz, fields in calls])
    for nz, fields in calls:
        y = run(handle, fields, nz, tail=16)
        w, m = held_to_yardstick(stack, features(stack, fields, nz), y, "%d->%r %s nz %d cells %d" % (n_in, widths, form, nz, fields[0].size), bounds)
        worst, misses, clipped = max(worst, w), misses + m, clipped + int((y[:, 1:] == 0).sum())
    handle.close()
    print("SHAPE %d->%r %s worst ratio %.3f" % (n_in, widths, form, worst))
    assert not misses, misses
    assert clipped > 0, "the clip never acted"


@pytest.mark.parametrize("form", ["state", "tendency"])
@pytest.mark.parametrize("ishape", range(len(SHAPES)))
def test_strict_kernel_is_the_index_order_statement(mw, ishape, form):
    from miniweatherml_amd import mlp
    n_in, widths = SHAPES[ishape]
    stack = make_stack(n_in, widths, form, ishape)
    handle = mlp.MlpStack(stack, "cuda")
    for nz, ncol in ((1, 1), (1, 17)) + (((3, 17),) if n_in == 9 else ()):
        fields = make_fields(nz * ncol, ishape)
        X = features(stack, fields, nz)
        assert np.array_equal(run(handle, fields, nz, strict=1, tail=16), unscale(stack, references(stack, X)[1], X))
    handle.close()


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("ishape", [9, 10, 12])
def test_a_nan_or_inf_cell_stays_alone(mw, ishape, strict):
    """One NaN, one +Inf and one -Inf cell inside a tile: every other cell of the call keeps the bits of the clean run (n_in = 9 at nz = 1,
    where no cell is another's level above)."""
    from miniweatherml_amd import mlp
    n_in, widths = SHAPES[ishape]
    handle = mlp.MlpStack(make_stack(n_in, widths, "tendency", ishape), "cuda")
    fields = make_fields(83, ishape)
    clean = run(handle, fields, 1, strict, tail=16)
    fields[0][5], fields[2][21], fields[4][22] = np.nan, np.inf, -np.inf
    dirty = run(handle, fields, 1, strict, tail=16)
    keep = np.ones(83, bool)
    keep[[5, 21, 22]] = False
    assert np.array_equal(dirty[keep].view(np.int64), clean[keep].view(np.int64))
    assert not np.array_equal(dirty[~keep].view(np.int64), clean[~keep].view(np.int64))
    handle.close()


def test_shipped_5_10_4_as_a_stack(mw):
    """The reference's shipped Keras file through stack_from_h5, held to the fp64 forward as mw_mlp_forward is (never kernel to kernel);
    n_in = 5 may write in place."""
    from miniweatherml_amd import mlp
    import os
    stack = mlp.stack_from_h5(os.path.join(mlp._DATA, "supercell_kessler_singlecell_model_weights.h5"), ("dense_6", "dense_7"), [0.1])
    assert mlp.stack_widths(stack) == [5, 10, 4]
    rng = np.random.default_rng(5)
    fields = [rng.uniform(lo, hi, 1000) for lo, hi in stack.scl_in]
    y = run(mlp.MlpStack(stack, "cuda"), fields, 1, tail=16)
    X = np.stack(fields, 1)
    assert not held_to_yardstick(stack, X, y, "shipped 5->10->4", shape_bound(stack, [X]))[1]
    dev = [torch.from_numpy(f).cuda() for f in fields]
    mlp.mlp_stack_forward(stack, 1, *dev, outs=[dev[0], dev[2], dev[3], dev[4]])
    assert np.array_equal(np.stack([dev[i].cpu().numpy() for i in (0, 2, 3, 4)], 1), y)


BAD = {"width 0": dict(widths=[0]), "width 65": dict(widths=[65]), "depth 0": dict(widths=[]), "depth 5": dict(widths=[8] * 5), "n_in 6": dict(n_in=6),
       "negative slope": dict(slopes=[-0.1]), "nan slope": dict(slopes=[np.nan]), "inf slope": dict(slopes=[np.inf]), "input row": dict(row_in=2),
       "output row": dict(row_out=1), "form 2": dict(form=2), "count": dict(extra=1)}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_create_refuses(mw, bad):
    from miniweatherml_amd import capi
    k = dict(dict(n_in=5, widths=[8], slopes=None, row_in=None, row_out=None, form=0, extra=0), **BAD[bad])
    w = [k["n_in"]] + k["widths"] + [4]
    slopes = np.array(k["slopes"] or [0.1] * len(k["widths"]), np.float32)
    params = np.zeros(sum((a + 1) * b for a, b in zip(w[:-1], w[1:])) + k["extra"], np.float32)
    scl_in, scl_out = np.array(BOX), np.array([[0., 1.]] * 4)
    if k["row_in"] is not None:
        scl_in[k["row_in"], 1] = scl_in[k["row_in"], 0]
    if k["row_out"] is not None:
        scl_out[k["row_out"], 1] = scl_out[k["row_out"], 0]
    h, fp, dp = C.c_void_p(), C.POINTER(C.c_float), C.POINTER(C.c_double)
    rc = capi.lib().mw_mlp_stack_create(C.byref(h), k["n_in"], len(k["widths"]), (C.c_int * 8)(*k["widths"]), slopes.ctypes.data_as(fp),
                                        params.ctypes.data_as(fp), params.size, scl_in.ctypes.data_as(dp),
                                        scl_out.ctypes.data_as(dp), k["form"])
    assert rc != 0 and not h.value and b"mlp_stack_create" in capi.lib().mw_last_error()


def test_nine_inputs_refuse_aliased_outputs(mw):
    from miniweatherml_amd import capi, mlp
    handle = mlp.MlpStack(make_stack(9, [10], "state", 0), "cuda")
    dev = [torch.from_numpy(f).cuda() for f in make_fields(34, 0)]
    with pytest.raises(capi.MWError, match="must not overlap"):
        handle.forward(2, *dev, outs=[dev[0], dev[2], dev[3], dev[4]])


@pytest.mark.parametrize("online", [False, True])
def test_stack_in_the_model_loop(mw, online):
    """Microphysics_Kessler_Surrogate.init(coupler, stack=...) on a 4 x 4 x 6 coupler with two members: after each of two steps the
    network's result -- and online the state -- is what mlp_stack_forward gives on the fields before the step."""
    from miniweatherml_amd import mlp, modules
    stack = make_stack(9, [17, 5], "tendency", 3)
    micro = modules.Microphysics_Kessler_Surrogate()
    init = micro.init
    micro.init = lambda c: init(c, stack=stack)                       # make_supercell calls init(coupler)
    coupler, dycore, micro = modules.make_supercell(4, 4, 6, 2, 2000., 2000., 20000., micro=micro)
    micro.online = online
    dm = coupler.get_data_manager_readwrite()
    names = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
    for _ in range(2):
        before = [dm.get(n).clone() for n in names]
        want = mlp.mlp_stack_forward(stack, 6, *before)
        got = micro.time_step(coupler, 1.0)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        if online:
            assert all(torch.equal(dm.get(n), w) for n, w in zip(mlp.OUT4, want))
        else:
            assert not torch.equal(dm.get("temp"), want[0])
