"""Keeps tests/test_gpu_column_edges.py and tests/test_gpu_output_edges.py honest, without a GPU:

  * the constants their shape lists were chosen around are read from the kernels' text (csrc/mw_column.hip, csrc/mw_output.hip), and the
    lists must still straddle every one of them -- a later change of SLICE, of a cells-per-thread count, of a block size or of a block cap
    fails here instead of silently moving the edges away from the shapes;
  * the exact-grid generator really is exact: forwards, backwards and in Python integers;
  * the numpy restatements give hand-computed values on two cells."""
import math
import os
import re

import numpy as np

import test_gpu_column_edges as col
import test_gpu_output_edges as outp

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "miniweatherml_amd", "csrc")
COLUMN_HIP = open(os.path.join(CSRC, "mw_column.hip")).read()
OUTPUT_HIP = open(os.path.join(CSRC, "mw_output.hip")).read()


def const(text, pattern):
    m = re.findall(pattern, text, flags=re.S)
    assert len(m) == 1, (pattern, m)
    return tuple(int(x) for x in m[0]) if isinstance(m[0], tuple) else int(m[0])


def block_of(text, kernel):
    return const(text, r"__launch_bounds__\((\d+)\)\s*void\s+%s\(" % kernel)


def straddles(values, edge):
    return edge - 1 in values and edge in values and edge + 1 in values


# ---- the kernels' constants ---------------------------------------------------------------------------------------------------------------
SLICE = const(COLUMN_HIP, r"static constexpr int SLICE\s*=\s*(\d+);")
SPONGE_NPT = const(COLUMN_HIP, r"static constexpr int SPONGE_NPT\s*=\s*(\d+);")
NUDGE_NPT = const(COLUMN_HIP, r"static constexpr int NUDGE_NPT\s*=\s*(\d+);")
CHAIN_LAST, CHAIN_STRIDE = const(COLUMN_HIP, r"for \(; c \+ (\d+) < c1; c \+= (\d+)\)")
TAIL_STRIDE = const(COLUMN_HIP, r"for \(; c < c1; c \+= (\d+)\)")
SPONGE_CACHED = const(COLUMN_HIP, r"sh_target\[(\d+)\];")


def hsum_loops(n, threads):
    """Cells of a slice of n cells that k_hsum_partial's four-chain loop and its tail loop add: (chain cells, tail cells), as the kernel's two
    for statements walk them."""
    chain, tail = [], []
    for t in range(threads):
        c = t
        while c + CHAIN_LAST < n:
            chain += [c + q * (CHAIN_STRIDE // 4) for q in range(4)]
            c += CHAIN_STRIDE
        while c < n:
            tail.append(c)
            c += TAIL_STRIDE
    return chain, tail


def slice_lengths(ncell):
    return [min(SLICE, ncell - c0) for c0 in range(0, ncell, SLICE)]


def test_horizontal_sum_shapes_straddle_the_kernels_edges():
    threads = block_of(COLUMN_HIP, "k_hsum_partial")
    assert (threads, TAIL_STRIDE, CHAIN_STRIDE, CHAIN_LAST) == (256, threads, 4 * threads, 3 * threads)
    assert SLICE % CHAIN_STRIDE == 0 and block_of(COLUMN_HIP, "k_hsum_finish") == 256
    cells = [ny * nx for ny, nx in col.AVERAGE_SHAPES]
    assert sorted(set(cells)) == sorted(set(col.L_TAIL + col.L_CHAINS + col.L_SLICES))
    assert col.SHAPE_3D[0] > 1 and col.SHAPE_3D[1] > 1 and col.SHAPE_3D[0] * col.SHAPE_3D[1] in col.L_SLICES
    # the model of the two loops adds every cell of a slice once
    for n in (1, CHAIN_LAST, CHAIN_LAST + 1, CHAIN_STRIDE + 1, 1793, SLICE):
        chain, tail = hsum_loops(n, threads)
        assert sorted(chain + tail) == list(range(n))
    # a wavefront, a block, the first length that enters the four-chain loop, one whole round of it, a slice, two slices
    for edge in (64, threads, CHAIN_STRIDE, SLICE):
        assert straddles(cells, edge), edge
    assert CHAIN_LAST in cells and CHAIN_LAST + 1 in cells
    assert 2 * SLICE in cells and 2 * SLICE + 1 in cells and SLICE + CHAIN_LAST + 1 in cells
    assert all(not hsum_loops(n, threads)[0] for n in col.L_TAIL) and max(col.L_TAIL) == CHAIN_LAST
    kinds = set()
    for n in cells:
        for ln in slice_lengths(n):
            chain, tail = hsum_loops(ln, threads)
            kinds.add((bool(chain), bool(tail)))
    assert kinds == {(False, True), (True, True), (True, False)}   # tail only; chains and a tail; chains that leave no tail
    assert all(hsum_loops(n, threads)[0] for n in col.L_CHAINS)
    assert {len(slice_lengths(n)) for n in cells} == {1, 2, 3}
    assert any(slice_lengths(n)[-1] == 1 for n in cells) and any(slice_lengths(n)[-1] == CHAIN_LAST + 1 for n in cells if n > SLICE)
    assert max(cells) <= 2 ** 16 and col.REAL_SUM_L == max(cells)   # (the exactness argument of exact_ints)


def test_sponge_shapes_straddle_the_block_and_the_cached_members():
    threads = block_of(COLUMN_HIP, "k_sponge_apply")
    block = threads * SPONGE_NPT
    assert (threads, block, SPONGE_CACHED) == (256, 1024, 64)
    elems = {nens: [n * e for n, e in col.SPONGE_CASES if e == nens] for nens in (1, 3)}
    assert straddles(elems[1], block)
    assert block - 3 < max(x for x in elems[3] if x < block) and min(x for x in elems[3] if x > block) < block + 3      # three members: the nearest
    members = [e for _, e in col.SPONGE_CASES]
    assert straddles(members, SPONGE_CACHED) and max(members) > 2 * SPONGE_CACHED
    assert any(n > SLICE and e == 1 for n, e in col.SPONGE_CASES)
    assert min(col.SPONGE_NZ) == col.SPONGE_LAYERS and col.SPONGE_LAYERS + 1 in col.SPONGE_NZ and max(col.SPONGE_NZ) > col.SPONGE_LAYERS + 1
    assert col.SPONGE_FIELDS == 8 and col.WFLD == 3


def test_nudge_shapes_straddle_the_block():
    threads = block_of(COLUMN_HIP, "k_nudge_apply")
    assert (threads, threads * NUDGE_NPT) == (256, 2048)
    assert straddles(col.NUDGE_L, threads) and straddles(col.NUDGE_L, threads * NUDGE_NPT) and 2 * threads * NUDGE_NPT + 1 in col.NUDGE_L
    assert col.NUDGE_NENS == (1, 2, 3)


def test_output_sizes_straddle_the_block_caps():
    for k in ("k_extract_member", "k_hsponge_apply", "k_active_count", "k_gather_samples", "k_diff_partial", "k_validate"):
        assert block_of(OUTPUT_HIP, k) == outp.BLOCK == 256, k
    cap, add, div = const(OUTPUT_HIP, r"int mw_mean_diff\(.*?std::min<long long>\((\d+), \(n \+ (\d+)\) / (\d+)\)")
    assert (cap, add + 1, div) == (outp.MEAN_CAP, outp.BLOCK, outp.BLOCK)
    cap, add, div = const(OUTPUT_HIP, r"static int validate_any\(.*?std::min<long long>\((\d+), \(n \+ (\d+)\) / (\d+)\)")
    assert (cap, add + 1, div) == (outp.VALIDATE_CAP, outp.BLOCK, outp.BLOCK)
    assert (outp.VALIDATE_CAP, outp.MEAN_CAP) == (4096, 1024)
    for sizes, span in ((outp.VALIDATE_N, outp.VALIDATE_SPAN), (outp.MEAN_N, outp.MEAN_SPAN)):
        assert span in (outp.VALIDATE_CAP * 256, outp.MEAN_CAP * 256)
        assert straddles(sizes, 256) and straddles(sizes, span) and max(sizes) > 2 * span and min(sizes) == 1
    assert straddles(outp.VALIDATE_N, 64)
    assert straddles(sorted(outp.ACTIVE_SHAPES), 64) and straddles(sorted(outp.ACTIVE_SHAPES), 256) and max(outp.ACTIVE_SHAPES) > 512
    assert all(nz * ny * nx == n for n, (nz, ny, nx) in outp.ACTIVE_SHAPES.items())
    # 7 x 5: from 4 cells on the centre column lies in both x strips, at 7 the strips cover the domain, at 9 they exceed it
    assert min(outp.HSPONGE_CELLS) == 2 and 2 * 4 > 7 >= 2 * 3 and {3, 4, 7, 9} <= set(outp.HSPONGE_CELLS)
    assert (1, 1, 1, 1) in outp.HSPONGE_FLAGS and all(tuple(int(i == s) for i in range(4)) in outp.HSPONGE_FLAGS for s in range(4))


def test_validator_plants_reach_every_pass_and_stay_inside():
    for n in outp.VALIDATE_N:
        plants = outp.validate_plants(n)
        names = [name for name, _ in plants]
        assert plants[0] == ("clean", []) and len(set(names)) == len(names)
        for name, p in plants:
            idx = [i for i, _ in p]
            assert all(0 <= i < n for i in idx) and len(set(idx)) == len(idx), (n, name)
        for kind in outp.KINDS:
            assert dict(plants)["%s at 0" % kind][0][0] == 0 and dict(plants)["%s at n - 1" % kind][0][0] == n - 1
            if n > outp.VALIDATE_SPAN:
                assert all(i >= outp.VALIDATE_SPAN for i, _ in dict(plants)["%s in the second pass only" % kind])
                (lo, _), (hi, _) = dict(plants)["%s: the lowest index in a higher block" % kind]
                blocks = [(i % outp.VALIDATE_SPAN) // outp.BLOCK for i in (lo, hi)]
                assert lo < hi and blocks[0] > blocks[1]
            if n >= 64:
                (a, _), (b, _) = dict(plants)["two %s in one wavefront" % kind]
                assert a != b and a // 64 == b // 64
    assert max(outp.VALIDATE_N) - 1 >= 2 * outp.VALIDATE_SPAN      # "at n - 1" of the largest size lies in a third pass


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def test_exact_grid_sums_do_not_depend_on_the_order():
    n = max(ny * nx for ny, nx in col.AVERAGE_SHAPES)
    ints = col.exact_ints(1, (2, n))
    assert ints.dtype == np.int64 and np.all(ints != 0) and np.abs(ints).max() <= 2 ** 20 and (ints > 0).any() and (ints < 0).any()
    assert not np.array_equal(ints[0], ints[1])
    vals = col.exact_values(ints)
    assert np.array_equal(vals * 1024.0, ints)
    for row in range(2):
        fwd = bwd = 0.0
        for x in vals[row].tolist():
            fwd += x
        for x in vals[row][::-1].tolist():
            bwd += x
        py = sum(int(k) for k in ints[row].tolist())
        assert fwd == bwd == py / 1024.0 == math.fsum(vals[row].tolist()) == col.exact_sums(ints, 1)[row]
        assert float(np.sort(np.abs(vals[row])).cumsum()[-1]) == sum(abs(int(k)) for k in ints[row].tolist()) / 1024.0
    assert 2 ** 16 * 2 ** 20 < 2 ** 53


# ---- the restatements on two cells --------------------------------------------------------------------------------------------------------
def test_column_average_ref_on_two_cells():
    ints = np.array([[[[1024 * (f + 1)], [-512]]] for f in range(5)], dtype=np.int64)          # (5, 1, 2, 1): f + 1 and -0.5
    assert col.column_average_ref(ints, 2, 1).tolist() == [[[0.25]], [[0.75]], [[1.25]], [[1.75]], [[2.25]]]
    assert col.column_average_ref(ints, 4, 2).tolist() == [[[0.0625]], [[0.1875]], [[0.3125]], [[0.4375]], [[0.5625]]]


def test_sponge_ref_on_two_cells():
    nz, zlen = 11, 11.0                                            # dz = 1: level k is (11 - k - 0.5) / 10 sponge depths below the top
    top, bottom = col.sponge_factor(10, nz, zlen, 6.0, 60.0), col.sponge_factor(1, nz, zlen, 6.0, 60.0)
    assert abs(top - 0.1 * 0.9938441702975689) < 1e-16 and abs(bottom - 0.1 * 0.0061558297024311) < 1e-16       # (cos(pi / 20) + 1) / 2 and 1 - that
    fields = np.zeros((col.SPONGE_FIELDS, nz, 2, 1))
    fields[:, :, 0, 0], fields[:, :, 1, 0] = 2.0, 4.0
    sums = np.full((col.SPONGE_FIELDS, col.SPONGE_LAYERS, 1), 6.0)
    got = col.sponge_ref(fields, sums, zlen, 6.0, 60.0, 2)
    assert np.array_equal(got[:, 0], fields[:, 0])                  # level 0 lies below the ten sponge levels
    for f in range(col.SPONGE_FIELDS):
        target = 0.0 if f == col.WFLD else 3.0
        assert got[f, 10, :, 0].tolist() == [2.0 + (target - 2.0) * top, 4.0 + (target - 4.0) * top]
        assert got[f, 1, :, 0].tolist() == [2.0 + (target - 2.0) * bottom, 4.0 + (target - 4.0) * bottom]
    assert got[0, 10, 0, 0] > 2.0 and got[0, 10, 1, 0] < 4.0 and got[col.WFLD, 10, 0, 0] < 2.0


def test_nudge_ref_on_two_cells():
    state = np.zeros((5, 1, 2, 1))
    state[:, 0, 0, 0], state[:, 0, 1, 0] = 1.0, 2.0
    column, avg = np.full((5, 1, 1), 7.0), np.full((5, 1, 1), 1.5)
    got = col.nudge_ref(state, column, avg, 5.0)
    assert got[:, 0, :, 0].tolist() == [[1.0 + 27.5 / 900.0, 2.0 + 27.5 / 900.0]] * 5


def test_output_refs_on_two_cells():
    assert outp.validate_ref(np.array([float("nan"), 1.0, -float("inf"), -0.0, -2.0, float("inf")])) == [1, 2, 2, 0, 2, 2]
    assert outp.validate_ref(np.array([0.0, -0.0], dtype=np.float32)) == [0, 0, 0, -1, -1, -1]
    assert outp.exact_mean_diff_ref(np.array([1024, 2048]), np.array([512, 512])) == 1.0
    in4, out4 = np.zeros((4, 2, 2)), np.zeros((4, 2, 2))
    out4[2, 1, 0], out4[:, 0, 1] = 2.0e-10, 5.0                       # cell 1 changes in member 0; cell 0 only in member 1
    assert outp.active_ref(in4, out4)[0] == 1 and outp.active_ref(in4, out4)[1].tolist() == [0, 1]
    out4[2, 1, 0] = 1.0e-10
    assert outp.active_ref(in4, out4)[0] == 0
    # two cells on top of each other: the lower one's stencil reaches the upper, the upper one's is clamped to itself
    rho_d = np.array([[1.5, 9.0], [2.5, 9.0]])
    f4 = np.array([[[10.0 * v + c, 99.0] for c in range(2)] for v in range(1, 5)])
    ins, outs = outp.gather_ref(rho_d, f4, -f4, np.array([0, 1]), 2, 1)
    assert ins.dtype == np.float32 and ins.tolist() == [[10, 11, 1.5, 21, 20, 31, 30, 41, 40, 0], [11, 11, 2.5, 21, 21, 31, 31, 41, 41, 0]]
    assert outs.tolist() == [[-10, -20, -30, -40], [-11, -21, -31, -41]]
    assert outp.gather_ref(rho_d, f4 + 1e-9, -f4, np.array([0]), 2, 1)[0][0, 0] == np.float32(10.000000001)


def test_horizontal_sponge_ref_on_two_cells():
    """nx = 2, ny = 1, two sponge cells, dt / time_scale = 1/4: the weight is 1/4 on a pass's own edge cell and (cos(pi) + 1) / 2 = 0 on the
    other, and both y passes see distance 0 everywhere.  v = (8, 16), column 4 -- every step is exact in binary."""
    fields = np.zeros((6, 1, 1, 2, 1))
    fields[..., 0, 0], fields[..., 1, 0] = 8.0, 16.0
    column = np.full((6, 1, 1), 4.0)
    run = lambda *fl, **kw: outp.hsponge_ref(fields, column, 2, 1.0, 0.25, *fl, **kw)[0, 0, 0, :, 0].tolist()    # noqa: E731
    assert run(1, 0, 0, 0) == [7.0, 16.0] and run(0, 1, 0, 0) == [8.0, 13.0]
    assert run(0, 0, 1, 0) == run(0, 0, 0, 1) == [7.0, 13.0]
    assert run(1, 1, 1, 1) == [5.6875, 9.0625]                     # 8 -> 7 -> 7 -> 6.25 -> 5.6875 and 16 -> 16 -> 13 -> 10.75 -> 9.0625
    assert run(1, 1, 0, 0, px=0, nproc_x=2) == [7.0, 16.0] and run(1, 1, 0, 0, px=1, nproc_x=2) == [8.0, 13.0]
    assert run(0, 0, 1, 1, py=1, nproc_y=3) == [8.0, 16.0]
