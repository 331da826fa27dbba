"""Committees of dense stacks (mw_stack_group_committee_apply): the mean and range of a selection of a group's stacks on
one ensemble member, against the numpy rule of committee_ref applied to MlpStack.forward of each selected stack."""
import functools

import numpy as np
import pytest
import torch

from committee_ref import combine, same_bits
from test_gpu_mlp_stack import features, make_stack, references, shape_bound, unscale
from test_gpu_stack_members import TAIL, bits, forward_of_member, member_fields

pytestmark = pytest.mark.gpu

W4 = [64, 64, 64, 64]
# "chunked": by the greedy rule {[3], 64^4}, {64^4}, {64^4, [3]} -- a first, a middle and a last launch; reversed, the same three
COMMITTEES = {"one": [(5, [17], "tendency")],
              "three5": [(5, [17], "tendency"), (5, [3], "state"), (5, [33], "state")],
              "three9": [(9, [10], "state"), (9, [17, 5], "tendency"), (9, [3], "state")],
              "sixteen": [(5, [1 + k % 5], "tendency" if k % 3 == 0 else "state") for k in range(16)],
              "chunked": [(5, [3], "state"), (5, W4, "tendency"), (5, W4, "state"), (5, W4, "state"), (5, [3], "tendency")]}
FLAT, COLS = [(1, 1, 1), (5, 17, 3), (4, 65, 5)], [(2, 15, 3), (4, 17, 1), (9, 65, 3)]
CASES = [(key, sh, rev) for key, rev in (("one", 0), ("three5", 0), ("three9", 0), ("sixteen", 0), ("chunked", 0), ("chunked", 1))
         for sh in (COLS if key == "three9" else FLAT)]
OWN = (0, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def stacks_of(key):
    return [make_stack(n_in, widths, form, seed) for seed, (n_in, widths, form) in enumerate(COMMITTEES[key])]


def rule(stacks, f5, e, strict=0):
    """[(mean, range)] per output field: committee_ref.combine of MlpStack.forward of every stack on member e."""
    ys = [[o.cpu().numpy() for o in forward_of_member(s, f5, e, strict)] for s in stacks]
    return [combine([y[v] for y in ys]) for v in range(4)]


def tailed_like(f):
    flat = torch.full((f.numel() + TAIL,), -7.5, dtype=torch.float64, device="cuda")
    return flat[:f.numel()].view(f.shape), flat


def check(group, sel, e, f5, flat5, want, in_place, with_range):
    """One committee_apply on clones of the state against `want`; the inputs it must not write, the other members and the tails keep
    their bits."""
    nz = f5[0].shape[0]
    g5 = [d.clone() for d in flat5]
    v5 = [d[:f.numel()].view(f.shape) for d, f in zip(g5, f5)]
    outs = [tailed_like(f5[0]) for _ in range(8)]
    out4 = [v5[i] for i in OWN] if in_place else [o[0] for o in outs[:4]]
    rng4 = [o[0] for o in outs[4:]] if with_range else None
    group.committee_apply(nz, sel, e, v5, out4, rng4)
    torch.cuda.synchronize()
    for v in range(4):
        assert same_bits(out4[v][..., e].cpu().numpy(), want[v][0]), ("mean", v, in_place, with_range)
        if with_range:
            assert same_bits(rng4[v][..., e].cpu().numpy(), want[v][1]), ("range", v, in_place)
    others = [m for m in range(f5[0].shape[-1]) if m != e]
    written = OWN if in_place else ()
    for i in range(5):
        assert torch.equal(bits(v5[i][..., others]), bits(f5[i][..., others])), "another member was written"
        assert i in written or torch.equal(bits(v5[i]), bits(f5[i])), "an input was written"
    for o, _ in outs:
        assert bool((o[..., others] == -7.5).all()), "another member of an output was written"
    assert all(bool((d[-TAIL:] == -7.5).all()) for d in g5 + [o[1] for o in outs]), "a cell behind an array was written"


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("key,shape,rev", CASES)
def test_bits_are_the_rule_on_the_forward_kernels(mw, key, shape, rev, strict):
    from miniweatherml_amd import mlp
    nz, ncol, nens = shape
    stacks = stacks_of(key)
    sel = list(range(len(stacks)))[::-1] if rev else list(range(len(stacks)))
    e = (nz + ncol) % nens
    f5, flat5 = member_fields(nz, ncol, nens, ncol)
    want = rule([stacks[j] for j in sel], f5, e, strict)
    group = mlp.MlpStackGroup(stacks, "cuda")
    group.strict = strict
    for in_place, with_range in ((0, 1), (1, 1), (1, 0), (0, 0)):
        check(group, sel, e, f5, flat5, want, in_place, with_range)
    if key == "one":
        assert all(np.array_equal(want[v][1], np.zeros((nz, ncol))) and not np.signbit(want[v][1]).any() for v in range(4))
    group.close()


def test_a_committee_of_one_keeps_minus_zero(mw):
    """A stack whose temp is -0.0 on every cell (a last layer of zeros gives +0, un-scaled by min -0 and range -1): the committee of one
    returns the sign, and range +0."""
    from miniweatherml_amd import mlp
    s = make_stack(5, [2], "state", 0)
    s = s._replace(layers=[s.layers[0], (np.zeros((2, 4), np.float32), np.zeros(4, np.float32))], scl_out=np.array([[-0.0, -1.0]] + s.scl_out[1:].tolist()))
    f5, flat5 = member_fields(2, 17, 2, 0)
    want = rule([s], f5, 1)
    assert np.signbit(want[0][0]).all() and not want[0][0].any()
    group = mlp.MlpStackGroup([s], "cuda")
    check(group, [0], 1, f5, flat5, want, 1, 1)
    group.close()


@pytest.mark.parametrize("n_in,nz,ncol", [(5, 1, 262145), (9, 2, 65537)])
def test_a_wave_makes_a_second_grid_stride_pass(mw, n_in, nz, ncol):
    """The grid is capped at 1024 workgroups of four waves.  Flat walk: a wave takes four 16-cell tiles per pass, so one grid pass covers
    1024 * 4 * 4 * 16 = 262,144 cells and cell 262,144 is wave 0's second pass.  Column walk: a wave takes 16 columns, one grid pass covers
    1024 * 4 * 16 = 65,536 columns and column 65,536 is wave 0's second pass."""
    from miniweatherml_amd import mlp
    stacks = [make_stack(n_in, [3], "state", 1), make_stack(n_in, [5], "tendency", 2)]
    f5, flat5 = member_fields(nz, ncol, 2, n_in)
    group = mlp.MlpStackGroup(stacks, "cuda")
    check(group, [1, 0], 1, f5, flat5, rule(stacks[::-1], f5, 1), 1, 1)
    group.close()


def test_the_order_of_sel_is_the_order_of_the_sum(mw):
    """Three stacks on a state where the numpy rule itself gives two different means for [0, 1, 2] and [2, 1, 0] (found on the host
    first): each order matches its own reference."""
    from miniweatherml_amd import mlp
    stacks = [make_stack(5, w, "tendency", k) for k, w in enumerate(([17], [3], [33]))]      # (base + change: the water fields' y have full mantissas)
    f5, flat5 = member_fields(5, 17, 1, 7)
    fwd, back = rule(stacks, f5, 0), rule(stacks[::-1], f5, 0)
    assert all(not same_bits(fwd[v][0], back[v][0]) for v in (1, 2, 3)), "the state does not tell the two orders apart"
    group = mlp.MlpStackGroup(stacks, "cuda")
    check(group, [0, 1, 2], 0, f5, flat5, fwd, 1, 1)
    check(group, [2, 1, 0], 0, f5, flat5, back, 0, 1)
    group.close()


def test_nan_weights_reach_temp_and_stop_at_the_clip(mw):
    from miniweatherml_amd import mlp
    stacks = list(stacks_of("three5"))
    stacks[1] = stacks[1]._replace(layers=[(W * np.float32(np.nan), b) for W, b in stacks[1].layers])
    f5, flat5 = member_fields(5, 17, 3, 5)
    group = mlp.MlpStackGroup(stacks, "cuda")
    out = [torch.zeros_like(f5[0]) for _ in range(8)]
    group.committee_apply(5, [0, 1, 2], 2, f5, out[:4], out[4:])
    assert bool(torch.isnan(out[0][..., 2]).all()) and bool(torch.isnan(out[4][..., 2]).all())
    assert all(bool(torch.isfinite(o[..., 2]).all()) for o in out[1:4] + out[5:])      # fmax(0, NaN) = 0 before combining
    check(group, [0, 2], 2, f5, flat5, rule([stacks[0], stacks[2]], f5, 2), 0, 1)
    group.close()


@pytest.mark.parametrize("n_in,form", [(5, "state"), (9, "tendency")])
def test_mean_against_fp64(mw, n_in, form):
    """nz = 5, ncol = 17, three stacks of one form (one output scaling): per field, in scaled space, |mean - mean of the fp64 forwards| <=
    the mean of the members' yardstick bounds (test_gpu_mlp_stack.shape_bound) + 2 ulp of fp64 of the largest mean.  The triangle
    inequality, and the clip at zero moves two values no further apart than they were, so both sides are clipped and no cell is left out.
    Worst ratio on the MI355X: 0.195 (n_in 5, state, temp), 0.137 (n_in 9, tendency, temp)."""
    from miniweatherml_amd import mlp
    stacks = [make_stack(n_in, w, form, k) for k, w in enumerate(([17], [33, 5], [64]))]
    f5, _ = member_fields(5, 17, 1, n_in)
    X = features(stacks[0], [f[..., 0].reshape(-1).cpu().numpy() for f in f5], 5)
    group = mlp.MlpStackGroup(stacks, "cuda")
    out = [torch.zeros_like(f5[0]) for _ in range(4)]
    group.committee_apply(5, [0, 1, 2], 0, f5, out)
    y = np.stack([o.reshape(-1).cpu().numpy() for o in out], 1)
    group.close()
    want = np.mean([unscale(s, references(s, X)[0], X) for s in stacks], 0)
    rng_o = stacks[0].scl_out[:, 1] - stacks[0].scl_out[:, 0]
    bound = np.mean([shape_bound(s, [X]) for s in stacks], 0) + 2 * np.spacing(np.abs(y).max(0)) / rng_o
    err = (np.abs(y - want) / rng_o).max(0)
    for v in range(4):
        print("n_in %d %s field %d: err %.3e bound %.3e ratio %.3f clipped %d" % (n_in, form, v, err[v], bound[v], err[v] / bound[v], (y[:, v] == 0).sum()))
    assert np.all(err <= bound), (err, bound)


def test_through_the_rollout_and_the_evaluator(mw):
    """Two stacks, their committee and persistence on a 6 x 5 x 4 coupler: after one time_step the committee member is committee_apply of
    its own state before, every other member is the same rollout's without the committee; CommitteeEvaluator on the stack group gives
    committee_score's rows of the rule's mean and range."""
    from test_gpu_surrogate_rollout import fields, same
    from miniweatherml_amd import modules, surrogate_eval
    from miniweatherml_amd.mlp import IN5, OUT4
    stacks = [("deep", make_stack(5, [17, 5], "tendency", 1)), ("wide", make_stack(5, [33], "state", 2))]
    runs = []
    for committees in ([("both", ["wide", "deep"])], [("both", ["wide", "deep"])], []):
        micro = modules.Microphysics_Rollout()
        micro.init = functools.partial(micro.init, models=[], persistence=True, committees=committees, stacks=stacks)
        runs.append(modules.make_supercell(6, 5, 4, 4 + len(committees), 3000., 2500., 20000., micro=micro))
    (c5, _, m5), (c0, _, _), (c4, _, m4) = [r[:3] for r in runs]
    assert m5.member_names == ["kessler", "both", "deep", "wide", "persistence"] and m5.stack_members == [2, 3]
    before = [fields(c5, IN5)[n].reshape(4, 30, 5) for n in IN5]
    want = rule([stacks[1][1], stacks[0][1]], before, 1)
    m5.time_step(c5, 1.0)
    m4.time_step(c4, 1.0)
    a, b = fields(c5), fields(c4)
    for v, n in enumerate(OUT4):
        assert same_bits(a[n][..., 1].reshape(4, 30).cpu().numpy(), want[v][0]), n
    for n in a:
        assert same(a[n][..., [0, 2, 3, 4]], b[n]), n
    # the evaluator: c0 holds the state before the step, c5 the state after it (every member is one more column)
    raw = surrogate_eval.CommitteeEvaluator(m5.stack_group, [1, 0]).accumulate(c0, c5)
    in5 = [fields(c0, IN5)[n] for n in IN5]
    ref = rule([stacks[1][1], stacks[0][1]], [t.reshape(4, -1, 1) for t in in5], 0)
    dev = lambda q: [torch.from_numpy(np.ascontiguousarray(r[q])).cuda().reshape(in5[0].shape) for r in ref]      # noqa: E731
    stats, counts, covered = surrogate_eval.committee_score(4, in5, [a[n] for n in OUT4], dev(0), dev(1))
    assert same_bits(raw[0][0], stats) and np.array_equal(raw[1], counts) and np.array_equal(raw[2], covered)


def test_entry_refusals(mw):
    from miniweatherml_amd import capi, mlp
    group = mlp.MlpStackGroup(stacks_of("three5") + stacks_of("three9")[:1] + stacks_of("chunked")[1:3], "cuda")
    f5, _ = member_fields(2, 3, 2, 0)
    out = [torch.zeros_like(f5[0]) for _ in range(8)]
    for sel, e, o4, r4, text in (([], 0, out[:4], None, "1 to 16 stacks, got 0"), (list(range(17)), 0, out[:4], None, "got 17"),
                                 ([0, 6], 0, out[:4], None, "stack 6 is outside"), ([1, 1], 0, out[:4], None, "stack 1 is given twice"),
                                 ([0, 3], 0, out[:4], None, "differ in n_in"), ([0], 2, out[:4], None, "member 2 is outside"),
                                 ([0], 0, [f5[2], out[1], out[2], out[3]], None, "its own input field"),
                                 ([0], 0, out[:4], [out[0]] + out[5:], "range field must not overlap an output")):
        with pytest.raises(capi.MWError, match=text):
            group.committee_apply(2, sel, e, f5, o4, r4)
    import ctypes as C
    L, n = capi.lib(), C.c_longlong(-1)
    sel = (C.c_int * 2)(4, 5)
    assert L.mw_stack_group_committee_workspace_bytes(group._h, 2, sel, 2, 3, C.byref(n)) == 0 and n.value == 96 * 6
    assert L.mw_stack_group_committee_workspace_bytes(group._h, 1, sel, 2, 3, C.byref(n)) == 0 and n.value == 0
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    rc = L.mw_stack_group_committee_apply(group._h, 2, sel, 0, 2, 3, 2, ptr(f5), ptr(out[:4]), None, None, 0, None)
    assert rc != 0 and b"needs a workspace of 576 bytes" in L.mw_last_error()
    group.close()
