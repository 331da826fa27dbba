"""Every layer shape of the dense stacks and a second grid pass, against numpy (csrc/mw_mlp_stack.h: stack_images, stack_dense,
stack_cells).  The references, the yardstick and its factor are test_gpu_mlp_stack.py's, unchanged.

1. SWEEP: one forward call per shape, production held to the yardstick and strict held to the fp32 index-order loop bit for bit.
   stack_images places unit u at row 4 (u % 4) + (u % 16) / 4 of block u / 16 and the next layer reads a[ki / 4][u][ki % 4]: the list
   holds every residue of n_i mod 4, every block count, and every block of a layer's last K step beside every block count of that
   layer (asserted below, at import).  n_in alternates 5 / 9 along the list and the form alternates along each n_in's own sub-list
   (state, state, tendency, tendency along the whole list), so that either n_in meets both forms in every class.  n_in = 5: nz = 1,
   509 cells (eight wave iterations of 64 cells over two workgroups, a partial last tile); n_in = 9: nz = 6, ncol = 85 (510 cells: the
   level above lies 85 cells on, never in the cell's own tile; the top level is its own level above).  The right-hand side is taken
   over a pool of 4096 cells of which the call's are the first.  The fp64 reference clips at most half of a call's cells per water
   field (asserted); SEEDS lists the shapes whose weights were drawn again for that.
2. Every sweep shape through k_stack_members and k_stack_eval, in groups of 32 per n_in: a member's bits are the forward kernel's,
   which part 1 holds to numpy; a group's rows are numpy's on the forward outputs (test_gpu_stack_eval.reference).
3. The second grid pass of k_mlp_stack and of k_stack_members' two walks.

Measured on an MI355X, the worst left / right of the yardstick over a class's shapes (printed by the tests as CLASS lines), state |
tendency, and the shape that gives it:
    depth 1  .366 5->[63]              .295 9->[64]
    depth 2  .424 9->[1, 64]           .386 5->[49, 33]
    depth 3  .477 5->[2, 31, 63]       .413 5->[1, 16, 64]
    depth 4  .474 9->[1, 64, 1, 64]    .378 5->[49, 3, 48, 16]
    second pass (every cell of the call)  .192 9->[3]  .242 5->[5]
The strict form has no ratio: its bits are the index-order loop's on every shape.  With an image builder that is wrong on purpose
(units 32..47 of a three-block layer at row r, not at 4 (r % 4) + r / 4) 43 production cases of part 1 fail, in every depth class,
and every other stack test of the suite passes, parts 2 and 3 here among them: they compare kernels that share the image.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_mlp_stack import features, held_to_yardstick, make_fields, make_stack, references, run, shape_bound, unscale
from test_gpu_stack_members import TAIL, bits, forward_of_member, member_fields, shuffled_members

pytestmark = pytest.mark.gpu

W = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
R = (1, 2, 3, 4, 16, 17, 33, 48, 49, 64)
POOL = 4096
GROUP = 32                                                        # MW_STACK_GROUP_MAX
# list index -> the seed of make_stack and make_fields where the index itself breaks the clip condition of part 1: the first of
# index + 1000 k that meets it (found on the host with the fp64 reference; 1000 k is a multiple of 4, so the slopes walk as the index's do).  The state
# form's water tables reach a fifth of their range below zero and a random network's outputs centre on zero, so most state shapes
# are here.
SEEDS = {0: 21000, 1: 60001, 4: 23004, 5: 9005, 8: 27008, 9: 6009, 10: 1010, 12: 88012, 13: 16013, 16: 3016, 17: 6017, 20: 30020, 21: 4021,
         24: 20024, 25: 21025, 26: 1026, 28: 158028, 29: 4029, 32: 70032, 33: 35033, 36: 55036, 37: 45037, 40: 12040, 41: 285041, 42: 1042,
         44: 352044, 45: 82045, 48: 57048, 49: 280049, 52: 250052, 53: 11053, 54: 2054, 56: 17056, 57: 99057, 60: 107060, 61: 249061, 63: 1063,
         64: 46064, 65: 12065, 68: 86068, 69: 27069, 72: 274072, 73: 29073, 76: 7076, 77: 138077, 79: 1079, 80: 17080, 81: 16081, 84: 117084,
         85: 1085, 86: 1086, 87: 1087, 88: 254088, 89: 9089, 92: 61092, 93: 92093, 96: 267096, 97: 108097, 100: 11100, 101: 97101, 104: 209104,
         105: 26105, 108: 130108, 109: 30109, 112: 54112, 113: 5113, 115: 1115, 116: 113116, 117: 50117, 118: 1118, 120: 118120, 121: 87121,
         124: 13124, 125: 25125, 128: 63128, 129: 10129, 132: 19132, 133: 6133, 136: 11136, 137: 15137, 140: 19140, 141: 13141, 143: 1143,
         144: 3144, 145: 42145, 148: 53148, 149: 154149, 151: 1151, 152: 9152, 153: 52153, 156: 6156, 157: 183157, 160: 45160, 161: 765161,
         164: 407164, 165: 66165, 168: 212168, 169: 382169, 172: 1516172, 173: 48173, 176: 108176, 177: 165177, 180: 246180, 181: 205181}


def _sweep():
    rng = np.random.default_rng(20241)
    shapes = [[w] for w in W for _ in (5, 9)] + [[a, b] for a in R for b in R]
    for depth in (3, 4):
        shapes += [[int(w) for w in rng.choice(W, depth)] for _ in range(24)]
    # a 64-wide layer read through one unit and back; the same twice; four block counts in falling order down to n_i = 2
    shapes += [[64, 1, 64], [1, 64, 1, 64], [49, 33, 17, 2]]
    return [((5, 9)[i % 2], w, ("state", "tendency")[i // 2 % 2], SEEDS.get(i, i)) for i, w in enumerate(shapes)]


SWEEP = _sweep()
CLASSES = {d: [i for i, s in enumerate(SWEEP) if len(s[1]) == d] for d in (1, 2, 3, 4)}


def _check_sweep():
    """What the sweep promises, so that a later edit of the list cannot quietly thin it."""
    assert {(s[0], s[1][0]) for s in SWEEP if len(s[1]) == 1} == {(n, w) for n in (5, 9) for w in W}
    assert sorted(tuple(s[1]) for s in SWEEP if len(s[1]) == 2) == sorted((a, b) for a in R for b in R)
    assert [len(CLASSES[d]) for d in (1, 2, 3, 4)] == [32, 100, 25, 26]
    assert len({(s[0], tuple(s[1])) for s in SWEEP}) == len(SWEEP)
    for d in CLASSES:
        assert {(SWEEP[i][0], SWEEP[i][2]) for i in CLASSES[d]} == {(n, f) for n in (5, 9) for f in ("state", "tendency")}
    hidden = [(a, b) for s in SWEEP for a, b in zip(s[1][:-1], s[1][1:])]      # layers that read units placed by stack_images
    last = [s[1][-1] for s in SWEEP]
    blocks = lambda n: (n + 15) // 16                                           # noqa: E731
    assert {a % 4 for a, _ in hidden} == {a % 4 for a in last} == {0, 1, 2, 3}
    assert {blocks(b) for _, b in hidden} == {blocks(s[1][0]) for s in SWEEP} == {1, 2, 3, 4}
    # the block of the layer's last K step ((ceil(n_i / 4) - 1) / 4) beside the layer's own block count
    assert {(((a + 3) // 4 - 1) // 4, blocks(b)) for a, b in hidden} == {(k, n) for k in range(4) for n in (1, 2, 3, 4)}
    assert {((a + 3) // 4 - 1) // 4 for a in last} == {0, 1, 2, 3}


_check_sweep()


def name(i):
    n_in, widths, form, _ = SWEEP[i]
    return "%d-%s-%s" % (n_in, "x".join(map(str, widths)), form)


def split(fields, n):
    return [f[:n] for f in fields], [f[n:] for f in fields]


@functools.lru_cache(maxsize=None)
def case(i):
    """Shape i of the sweep, computed once and never written: (stack, nz, the call's fields, the call's features X, (o_fp64, o_fp32loop)
    of the call's cells, the yardstick's right-hand side over the pool)."""
    n_in, widths, form, seed = SWEEP[i]
    stack = make_stack(n_in, widths, form, seed)
    nz, n = (1, 509) if n_in == 5 else (6, 6 * 85)
    call, rest = split(make_fields(POOL, seed), n)
    X = features(stack, call, nz)
    pool = np.concatenate([X, features(stack, rest, 11)])                       # (4096 - 510 = 11 * 326: ten levels of eleven have one above)
    return stack, nz, call, X, references(stack, X), shape_bound(stack, [pool])


def clipped_by_the_reference(stack, X, o64):
    """Cells per water field that the fp64 reference clips."""
    return (unscale(stack, o64, X, clip=False)[:, 1:] < 0).sum(0)


WORST = {}


def class_ratio(what, depth, form, ratio, shape):
    w = WORST.setdefault((what, depth, form), (0.0, ""))
    if ratio >= w[0]:
        WORST[(what, depth, form)] = (ratio, shape)
    print("CLASS %s depth %d %s: worst ratio so far %.3f at %s" % ((what, depth, form) + WORST[(what, depth, form)]))


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=name)
def test_production_kernel_against_fp64(mw, i):
    from miniweatherml_amd import mlp
    stack, nz, call, X, (o64, _), bounds = case(i)
    assert np.all(2 * clipped_by_the_reference(stack, X, o64) <= X.shape[0]), "the reference clips more than half of a water field"
    handle = mlp.MlpStack(stack, "cuda")
    y = run(handle, call, nz, tail=16)
    handle.close()
    worst, misses = held_to_yardstick(stack, X, y, name(i), bounds)
    class_ratio("production", len(SWEEP[i][1]), stack.form, worst, name(i))
    assert not misses, misses


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=name)
def test_strict_kernel_is_the_index_order_statement(mw, i):
    from miniweatherml_amd import mlp
    stack, nz, call, X, (_, o32), _ = case(i)
    handle = mlp.MlpStack(stack, "cuda")
    y = run(handle, call, nz, strict=1, tail=16)
    handle.close()
    assert np.array_equal(y, unscale(stack, o32, X))


# ---- 2. every sweep shape through the group kernels ----
GROUPS = [(n_in, k, idx[k:k + GROUP]) for n_in in (5, 9) for idx in ([i for i, s in enumerate(SWEEP) if s[0] == n_in],)
          for k in range(0, len(idx), GROUP)]
GROUP_IDS = ["%d-from-%d" % g[:2] for g in GROUPS]


def group_stacks(g):
    return [make_stack(*SWEEP[i]) for i in GROUPS[g][2]]


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("g", range(len(GROUPS)), ids=GROUP_IDS)
def test_member_bits_are_the_forward_kernels(mw, g, strict):
    """nz = 6, ncol = 21, one member per stack of the group, shuffled: a partial tile of cells and of columns, a level carried across
    two passes of four; the images at their img_off in the packed buffer, with the mpb the LDS plan picks."""
    from miniweatherml_amd import mlp
    stacks = group_stacks(g)
    nz, ncol, nens = 6, 21, len(stacks)
    members = shuffled_members(nens, nens, g)
    f5, flat = member_fields(nz, ncol, nens, g)
    before = [f.clone() for f in f5]
    want = [forward_of_member(s, before, e, strict) for s, e in zip(stacks, members)]
    group = mlp.MlpStackGroup(stacks, "cuda")
    group.members_apply(nz, members, f5, strict=strict)
    torch.cuda.synchronize()
    group.close()
    for i, w, e in zip(GROUPS[g][2], want, members):
        for v, f in enumerate((0, 2, 3, 4)):
            assert torch.equal(bits(f5[f][..., e]), bits(w[v])), (name(i), e, f)
    assert torch.equal(bits(f5[1]), bits(before[1])), "density_dry was written"
    assert all(bool((d[-TAIL:] == -7.5).all()) for d in flat), "a cell behind an array was written"


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=GROUP_IDS)
def test_group_rows_are_numpy_on_the_forward(mw, g):
    """One evaluate call on a 6 x 21 state: maxima and counts exact, sums to test_gpu_stack_eval.reference's bound."""
    from test_gpu_stack_eval import BEFORE, reference, state
    from miniweatherml_amd import mlp
    stacks = group_stacks(g)
    in5, truth4 = state(6, 21)
    group = mlp.MlpStackGroup(stacks, "cuda:0")
    got, counts = group.evaluate(6, in5, truth4)
    group.close()
    assert got.shape == (len(stacks) + 1, 2, 4, 4)
    preds = [forward_of_member(s, [f[..., None] for f in in5], 0, 0) for s in stacks] + [[in5[b] for b in BEFORE]]
    for m, pred in enumerate(preds):
        stats, bound, cnt = reference(pred, in5, truth4)
        assert np.array_equal(counts, cnt) and cnt.min() > 0, (m, counts, cnt)
        assert np.array_equal(got[m, :, :, 3], stats[:, :, 3]), (m, "max", got[m, :, :, 3], stats[:, :, 3])
        assert np.all(np.abs(got[m, :, :, :3] - stats[:, :, :3]) <= bound), (m, got[m], stats, bound)


# ---- 3. a second grid pass ----
SMALL = {"3-state": ([3], "state", 1150), "5-tendency": ([5], "tendency", 2)}      # (seeds whose reference clips under half of a field)


@pytest.mark.parametrize("key", sorted(SMALL))
@pytest.mark.parametrize("n_in,nz,ncol", [(5, 1, 524289), (9, 2, 262145)])
def test_forward_second_grid_pass(mw, n_in, nz, ncol, key):
    """mw_mlp_stack_forward launches min(ceil(waves / 4), STACK_MAX_BLOCKS = 2048) workgroups of four waves, a wave takes STACK_TILES =
    4 tiles of 16 cells per iteration and strides by gridDim.x * 4 waves: one pass of the full grid is 2048 * 4 * 4 * 16 = 524288
    cells, and cell 524288 is the first of tile 32768 = wave 0's t0 of its second iteration.  nz = 1, ncol = 524289 has that one cell
    there; nz = 2, ncol = 262145 has two, both of the top level, whose level below reads them from the first pass.  Every cell is held
    to the yardstick, whose right-hand side is over the call's own cells.  The strict kernel's grid is not capped (a thread per cell):
    its bits only guard the comparison."""
    from miniweatherml_amd import mlp
    widths, form, seed = SMALL[key]
    stack = make_stack(n_in, widths, form, seed)
    fields = make_fields(nz * ncol, seed)
    X = features(stack, fields, nz)
    o64, o32 = references(stack, X)
    assert np.all(2 * clipped_by_the_reference(stack, X, o64) <= X.shape[0])
    handle = mlp.MlpStack(stack, "cuda")
    y, ys = run(handle, fields, nz, tail=16), run(handle, fields, nz, strict=1, tail=16)
    handle.close()
    bounds = 4 * np.abs(o32 - o64).max(0) + 2.0 ** -23 * np.abs(o64).max(0)     # shape_bound(stack, [X]), from the references at hand
    worst, misses = held_to_yardstick(stack, X, y, "%d->%r %s %d x %d" % (n_in, widths, form, nz, ncol), bounds)
    class_ratio("second pass", 1, form, worst, "%d-%s" % (n_in, key))
    assert not misses, misses
    assert np.array_equal(ys, unscale(stack, o32, X))


FOUR = [([3], "state"), ([5], "tendency"), ([17], "state"), ([2, 3], "tendency")]


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in,nz,ncol", [(5, 1, 131073), (9, 5, 32769)])
def test_members_second_grid_pass(mw, n_in, nz, ncol, strict):
    """Four stacks of one n_in fit the LDS together, so stack_list_plan gives mpb = 4 and 4 / mpb = 1 tile slot per workgroup, and
    mw_stack_group_members_apply launches min(items, SM_MAX_BLOCKS = 2048) workgroups in x.  n_in = 5, the flat walk: an item is
    SM_TILES = 4 tiles of 16 cells, one pass is 2048 * 4 * 16 = 131072 cells, and nz = 1, ncol = 131073 puts one cell into block 0's
    second iteration.  n_in = 9, the column walk: an item is a tile of 16 columns, one pass is 2048 * 16 = 32768 columns, and ncol =
    32769 puts one column into block 0's second iteration; nz = 5 carries a level across two passes of four there.  The reference is
    the forward kernel on each member, a single pass of its own grid (131073 and 163845 cells), which part 1 holds to numpy.  The
    strict form runs as the comparison's guard only: its grid is capped at 2048 blocks of 256 columns, 524288 columns, which no test
    of a few seconds reaches."""
    from miniweatherml_amd import mlp
    stacks = [make_stack(n_in, w, form, k) for k, (w, form) in enumerate(FOUR)]
    members = shuffled_members(4, 4, nz)
    f5, flat = member_fields(nz, ncol, 4, n_in)
    before = [f.clone() for f in f5]
    want = [forward_of_member(s, before, e, strict) for s, e in zip(stacks, members)]
    group = mlp.MlpStackGroup(stacks, "cuda")
    group.members_apply(nz, members, f5, strict=strict)
    torch.cuda.synchronize()
    group.close()
    for w, e in zip(want, members):
        for v, f in enumerate((0, 2, 3, 4)):
            assert torch.equal(bits(f5[f][..., e]), bits(w[v])), (e, f)
    assert torch.equal(bits(f5[1]), bits(before[1])), "density_dry was written"
    assert all(bool((d[-TAIL:] == -7.5).all()) for d in flat), "a cell behind an array was written"
