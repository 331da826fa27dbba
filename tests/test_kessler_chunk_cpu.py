"""CPU-only: the z-chunk rule of the Kessler sweep (mw_kessler_chunk) against a Python restatement, the workspace bound that rests on
it, the three chunk lengths the benchmark configurations run with, and the test aid mw_kessler_debug_set_chunk."""
import pytest

CHUNKS = (25, 20, 16, 12, 10, 8, 5, 4)
COLUMNS = (1, 64, 65, 4096, 40_000, 160_000, 524_288, 1_000_000, 1_920_000, 2 ** 31)
NZ = range(2, 301)


def rule(nz, columns):
    """kessler_chunk (csrc/mw_kessler.hip): the longest list value below nz at which (wavefronts per level) x (chunks) reaches 16384,
    else the shortest list value below nz, else the whole column."""
    chunk = nz
    for c in CHUNKS:
        if c < nz:
            chunk = c
            if ((columns + 63) // 64) * ((nz + c - 1) // c) >= 16384:
                break
    return chunk


def test_rule_equals_its_restatement(mw):
    from miniweatherml_amd import capi
    L = capi.lib()
    for columns in COLUMNS:
        for nz in NZ:
            assert L.mw_kessler_chunk(nz, columns) == rule(nz, columns), (nz, columns)


def test_rule_keeps_the_workspace_bound(mw):
    """The result is the whole column or a list value below nz, and the chunk tops -- the flux_top rows a sweep writes and reads, one per
    chunk but the top one -- number at most nz / 4: inside the nz / 4 + 1 rows both workspace formulas reserve."""
    from miniweatherml_amd import capi
    L = capi.lib()
    for columns in COLUMNS:
        for nz in NZ:
            chunk = L.mw_kessler_chunk(nz, columns)
            assert chunk == nz or (chunk in CHUNKS and chunk < nz), (nz, columns, chunk)
            assert (nz + chunk - 1) // chunk - 1 <= nz // 4, (nz, columns, chunk)
    # the rows are in the formulas: the production workspace is 16 + (5 nz + nz / 4 + 1) ncol doubles, the teacher's 512 bytes more than
    # (nz + nz / 4 + 1) ncol nens doubles
    for nz, ncol in ((2, 1), (9, 257), (53, 549), (100, 160_000)):
        assert L.mw_kessler_workspace_bytes(nz, ncol) == 8 * (16 + 5 * nz * ncol + (nz // 4 + 1) * ncol)
        assert L.mw_kessler_members_teacher_workspace_bytes(nz, ncol, 3) == 512 + 8 * (nz + nz // 4 + 1) * ncol * 3


@pytest.mark.parametrize("nz,columns,chunk", [(50, 160_000, 8), (100, 160_000, 16), (60, 1_000_000, 25)])
def test_chunk_lengths_of_the_benchmark_configurations(mw, nz, columns, chunk):
    from miniweatherml_amd import capi
    assert rule(nz, columns) == chunk
    assert capi.lib().mw_kessler_chunk(nz, columns) == chunk


def test_rule_gives_four_at_the_shapes_of_the_small_tests(mw):
    """Why tests/test_gpu_kessler_edges.py needs the override: below 16384 (wavefront, chunk) pairs the rule runs to the end of its list."""
    from miniweatherml_amd import capi
    for nz, columns in ((20, 192), (40, 40), (53, 549), (26, 270)):
        assert capi.lib().mw_kessler_chunk(nz, columns) == 4


def test_debug_set_chunk_accepts_and_rejects(mw):
    from miniweatherml_amd import capi
    L = capi.lib()
    try:
        for ok in CHUNKS + (1024, 1025, 2 ** 20, 2 ** 31 - 1, 0):
            assert L.mw_kessler_debug_set_chunk(ok) == 0, ok
        for bad in (-1, -4, 1, 2, 3, 6, 7, 9, 11, 15, 24, 26, 50, 100, 1023, -(2 ** 31)):
            assert L.mw_kessler_debug_set_chunk(bad) != 0, bad
            assert "kessler_debug_set_chunk" in L.mw_last_error().decode() and str(bad) in L.mw_last_error().decode()
            with pytest.raises(capi.MWError, match="flux_top"):
                capi.check(L.mw_kessler_debug_set_chunk(bad))
        # the override does not touch what mw_kessler_chunk reports: that is the rule
        capi.check(L.mw_kessler_debug_set_chunk(25))
        assert L.mw_kessler_chunk(100, 160_000) == 16
    finally:
        capi.check(L.mw_kessler_debug_set_chunk(0))
