"""The production Kessler kernels (csrc/mw_kessler.hip) against the fp64 CPU oracle where the rest of the suite does not look: every
z-chunk length of the rainsplit == 1 sweep (mw_kessler_debug_set_chunk; the rule itself gives 4 at every small shape), wavefronts that
are rain-free, rainy or mixed, more than one workgroup of columns with a partial last one, nz at the edges of the chunk rule, the
alternating minimum words over calls of unequal weight, and buffer edges.

The state has 549 columns (61 x 9: two full workgroups and one of 37 lanes) and its rain and cloud are placed per wavefront (column //
64), see edge_state.  Comparisons with the oracle: 1e-12 relative to max|field| through util.compare_fields, the tolerance of the
kernels' header and of test_kessler_matches_oracle.  "Bit-identical" is equality of the uint64 views."""
import ctypes as C

import numpy as np
import pytest

from util import compare_fields

pytestmark = pytest.mark.gpu

NX, NY = 61, 9
NCOL = NX * NY                                                     # 549 = 8 wavefronts of 64 columns + one of 37
CHUNKS = (25, 20, 16, 12, 10, 8, 5, 4)                             # kessler_chunk's list
SINGLE = 1024                                                      # mw_kessler_debug_set_chunk: one chunk
NAMES = ("temp", "tracer0", "tracer1", "tracer2")                  # temp, rho_v, rho_c, rho_r in the oracle's naming
LIGHT, HEAVY = 5.0e-4, 2.0e-2                                      # rain amplitudes (test_gpu_kessler_mlp.rainy_state's)
SENTINEL = -777.25


# ---- the state --------------------------------------------------------------------------------------------------------------------------
_STATES = {}


def edge_state(oracle, nz, amp=LIGHT):
    """(nz, 549) arrays rho_d, temp, rho_v, rho_c, rho_r of an oracle supercell column set with test_gpu_kessler_mlp.rainy_state's draws
    (vapour scaled by U(0.6, 1.3), cloud U(0, 3e-3) in 60 % of the cells, rain U(0, amp) in half of them), then rain and cloud replaced
    per wavefront w = column // 64:
      0, 1  no rain and no cloud anywhere            2  rain in every lane, in the lower half of the levels only
      3     rain in lane 17 only, at all levels      4  cloud above the autoconversion threshold (1e-3), no rain
      6     rain on levels 0 and nz - 1 only         5, 7, 8 (37 lanes)  the per-cell draws
    plus dz and the dycore's CFL time step.  Cached; the arrays are read-only."""
    key = (nz, amp)
    if key in _STATES:
        return _STATES[key]
    dyc, f = oracle.supercell_setup(NX, NY, nz, 1, 500.0 * NX, 500.0 * NY, 20000.)
    rng = np.random.default_rng(11)
    shp = (nz, NCOL)
    rho_d = np.ascontiguousarray(f.rho_d.reshape(shp))
    qc = rng.uniform(0, 3e-3, shp) * (rng.uniform(size=shp) > 0.4)
    qr_all = rng.uniform(0, amp, shp)
    qr = qr_all * (rng.uniform(size=shp) > 0.5)
    rho_v = f.tracers[0].reshape(shp) * rng.uniform(0.6, 1.3, shp)
    wave, lane = np.arange(NCOL) // 64, np.arange(NCOL) % 64
    lev = np.arange(nz)[:, None]
    qc[:, wave <= 1] = 0.0
    qr[:, wave <= 1] = 0.0
    w = wave == 2
    qr[:, w] = (qr_all * (lev < max(1, nz // 2)))[:, w]
    w = wave == 3
    qr[:, w] = (qr_all * (lane == 17)[None, :])[:, w]
    w = wave == 4
    qc[:, w] = rng.uniform(1.2e-3, 3e-3, shp)[:, w]
    qr[:, w] = 0.0
    w = wave == 6
    qr[:, w] = (qr_all * ((lev == 0) | (lev == nz - 1)))[:, w]
    st = {"rho_d": rho_d, "temp": np.ascontiguousarray(f.temp.reshape(shp)), "rho_v": np.ascontiguousarray(rho_v), "rho_c": qc * rho_d,
          "rho_r": qr * rho_d}
    for a in st.values():
        a.flags.writeable = False
    st["dz"], st["dt_cfl"] = 20000. / nz, float(dyc.compute_time_step())
    dyc.close()
    _STATES[key] = st
    return st


def check_premises(st):
    """Rain-free, rainy and mixed wavefronts exist, level by level, and so do the cloud-free ones."""
    nz = st["rho_r"].shape[0]
    rain = np.zeros((nz, 9 * 64), dtype=bool)
    rain[:, :NCOL] = st["rho_r"] != 0.0
    per_wave = rain.reshape(nz, 9, 64).sum(axis=2)
    lanes = np.array([64] * 8 + [37])
    assert (per_wave[:, :2] == 0).all() and (per_wave[:, 4] == 0).all()                   # rain-free at every level
    assert (per_wave[0, 2] == 64) and (per_wave[nz - 1, 2] == 0)                          # all lanes below, none on top
    assert (per_wave[:, 3] == 1).all()                                                    # one lane
    assert ((per_wave[:, [5, 7, 8]] > 0) & (per_wave[:, [5, 7, 8]] < lanes[[5, 7, 8]])).any()    # mixed by chance
    assert per_wave[0, 6] == 64 and per_wave[nz - 1, 6] == 64 and (nz <= 2 or (per_wave[1:nz - 1, 6] == 0).all())
    assert not st["rho_c"][:, :128].any() and (st["rho_c"][:, 256:320] > 1.0e-3 * st["rho_d"][:, 256:320]).all()


_REFS = {}


def reference(oracle, st, dt, cols=None, key=None):
    """oracle.kessler_time_step on the state (or on its columns `cols`): ({name: (nz, ncol)}, precl, rainsplit), cached under `key`."""
    if key is not None and key in _REFS:
        return _REFS[key]
    a = {n: np.array(st[n] if cols is None else st[n][:, cols], order="C") for n in ("rho_v", "rho_c", "rho_r", "rho_d", "temp")}
    precl = np.zeros(a["temp"].shape[1])
    rs = oracle.kessler_time_step(st["dz"], dt, a["rho_v"], a["rho_c"], a["rho_r"], a["rho_d"], a["temp"], precl)
    out = ({"temp": a["temp"], "tracer0": a["rho_v"], "tracer1": a["rho_c"], "tracer2": a["rho_r"]}, precl, int(rs))
    for x in list(out[0].values()) + [precl]:
        x.flags.writeable = False
    if key is not None:
        _REFS[key] = out
    return out


# ---- the library call -------------------------------------------------------------------------------------------------------------------
def set_chunk(chunk):
    from miniweatherml_amd import capi
    capi.check(capi.lib().mw_kessler_debug_set_chunk(int(chunk)))


def overrides(nz):
    """The rule's own choice (0), every list value below nz, one chunk."""
    return [0] + [c for c in sorted(CHUNKS) if c < nz] + [SINGLE]


def kessler(st, dt, cols=None):
    """mw_kessler_time_step on the state's (nz, ncol) arrays with a fresh workspace: ({name: array}, precl, rainsplit)."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    t = {n: torch.from_numpy(np.array(st[n] if cols is None else st[n][:, cols], order="C")).cuda() for n in ("rho_v", "rho_c", "rho_r", "rho_d", "temp")}
    nz, ncol = t["temp"].shape
    precl = torch.full((ncol,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.mw_kessler_workspace_bytes(nz, ncol) // 8, dtype=torch.float64, device="cuda")
    rs = C.c_int(0)
    capi.check(L.mw_kessler_time_step(nz, ncol, st["dz"], float(dt), *[C.c_void_p(t[k].data_ptr()) for k in ("rho_v", "rho_c", "rho_r", "rho_d", "temp")],
                                      C.c_void_p(precl.data_ptr()), C.c_void_p(ws.data_ptr()), C.byref(rs), None))
    assert np.array_equal(t["rho_d"].cpu().numpy(), st["rho_d"] if cols is None else st["rho_d"][:, cols])
    return ({"temp": t["temp"].cpu().numpy(), "tracer0": t["rho_v"].cpu().numpy(), "tracer1": t["rho_c"].cpu().numpy(),
             "tracer2": t["rho_r"].cpu().numpy()}, precl.cpu().numpy(), rs.value)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def assert_same_bits(got, want, what):
    for n in NAMES:
        assert same_bits(got[0][n], want[0][n]), "%s: %s differs in %d cells" % (what, n, int((got[0][n] != want[0][n]).sum()))
    assert same_bits(got[1], want[1]), "%s: precl differs" % (what,)
    assert got[2] == want[2], what


def precl_close(got, want, what):
    err, lim = float(np.max(np.abs(got - want))), 1e-12 * max(float(np.max(np.abs(want))), 1e-300)
    print("%s: precl max|diff| %.3e, limit %.3e" % (what, err, lim))
    assert np.all(np.isfinite(got)) and err <= lim, what


def steps(st):
    """The dycore's CFL step; 20 s, where at nz >= 21 the upper levels are no longer "proven harmless" and the CFL pass evaluates the
    fall speed although the sub-cycle count stays 1; and dz / 37.5 s, which puts the limit 0.8 dz / dt at 30 m/s at ANY nz: below the
    bound 36.34 sqrt(rho0 / rho) of every cell (none is proven), above what rain of 5e-4 really falls at (the count stays 1)."""
    dt = st["dz"] / 37.5
    lim = 0.8 * st["dz"] / dt
    assert not ((36.34 * 36.34) * st["rho_d"][0] * (1.0 + 1.0e-9) < lim * lim * st["rho_d"]).any()
    return (("cfl", st["dt_cfl"]), ("20s", 20.0), ("unproven", dt))


NZS = (2, 4, 5, 9, 21, 26, 53)


# ---- 1, 2. every chunk length: against the oracle, and against one chunk ---------------------------------------------------------------
@pytest.mark.parametrize("nz", NZS)
def test_every_chunk_length_matches_the_oracle_and_one_chunk(mw, oracle, nz):
    """nz = 2 (the minimum: level nz - 1 sediments with zm), 4 (one chunk, no flux_top), 5 (a top chunk of one level), 21 and 26 (a chunk
    top is the first and only valid level of a 5-level group of the CFL pass), 9 and 53.  Every chunk length gives the oracle's result
    to 1e-12 AND the bits of the single-chunk sweep: flux_top is flux_here's expression on the same inputs, and the teacher's promise
    (its chunk comes from ncol * nens, Kessler alone's from ncol) rests on exactly that."""
    st = edge_state(oracle, nz)
    check_premises(st)
    try:
        for tag, dt in steps(st):
            ref, ref_precl, ref_rs = reference(oracle, st, dt, key=(nz, LIGHT, tag))
            assert ref_rs == 1 and ref_precl.max() > 0.0 and (ref_precl == 0.0).any()
            assert (ref["tracer2"][:, 256:320] != 0.0).any()                       # wavefront 4: rain comes in as zero and goes out non-zero
            assert all(np.all(np.isfinite(a)) for a in ref.values())
            set_chunk(SINGLE)
            one = kessler(st, dt)
            for ov in overrides(nz):
                set_chunk(ov)
                got = kessler(st, dt)
                what = "kessler edges nz=%d dt=%s chunk override %d" % (nz, tag, ov)
                assert got[2] == ref_rs == 1, what
                compare_fields(got[0], ref, 1e-12, what)
                precl_close(got[1], ref_precl, what)
                assert_same_bits(got, one, what + " against one chunk")
    finally:
        set_chunk(0)


# ---- 3. neighbours -----------------------------------------------------------------------------------------------------------------------
def test_neighbours_do_not_change_a_bit(mw, oracle):
    """The wave-uniform short cuts return exactly what the formulas return: a column's result does not depend on which columns share its
    wavefront.  A fixed permutation scatters the rainy columns of wavefronts 2-8 over wavefronts 0-1 and the reverse."""
    nz = 26
    st = edge_state(oracle, nz)
    perm = np.random.default_rng(5).permutation(NCOL)
    into_dry = (perm[:128] >= 128).sum()                                           # columns of wavefronts 2-8 that land in 0-1
    assert 64 <= into_dry and (perm[128:] < 128).sum() == into_dry
    ps = {n: (np.ascontiguousarray(st[n][:, perm]) if isinstance(st[n], np.ndarray) else st[n]) for n in st}
    try:
        for tag, dt in steps(st):
            for ov in (4, 16):
                set_chunk(ov)
                want = kessler(st, dt)
                got = kessler(ps, dt)
                assert got[2] == want[2] == 1
                back = ({n: np.empty_like(got[0][n]) for n in NAMES}, np.empty_like(got[1]), got[2])
                for n in NAMES:
                    back[0][n][:, perm] = got[0][n]
                back[1][perm] = got[1]
                assert_same_bits(back, want, "permuted columns, dt=%s chunk %d" % (tag, ov))
    finally:
        set_chunk(0)


# ---- 4. sub-cycling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", [5, 21, 53])
def test_sub_cycling_on_the_same_layout(mw, oracle, nz):
    """Rain of up to 2e-2: dt = 0.1 s per metre of dz (95 s at nz = 21) makes the fastest rain cross 0.8 dz several times; the count is the
    oracle's, the fields are the oracle's to 1e-12, and the chunk override -- the column sweep has no chunks -- changes nothing."""
    st = edge_state(oracle, nz, HEAVY)
    check_premises(st)
    dt = 0.1 * st["dz"]
    ref, ref_precl, ref_rs = reference(oracle, st, dt, key=(nz, HEAVY, "heavy"))
    print("nz = %d: dt = %.2f s, the oracle sub-cycles %d times" % (nz, dt, ref_rs))
    assert 2 <= ref_rs <= 8 and ref_precl.max() > 0.0
    try:
        first = None
        for ov in (0, 4, SINGLE):
            set_chunk(ov)
            got = kessler(st, dt)
            what = "kessler edges sub-cycling nz=%d chunk override %d" % (nz, ov)
            assert got[2] == ref_rs, what
            compare_fields(got[0], ref, 1e-12, what)
            precl_close(got[1], ref_precl, what)
            first = first or got
            assert_same_bits(got, first, what + " against no override")
    finally:
        set_chunk(0)


# ---- 5. the alternating minimum words ----------------------------------------------------------------------------------------------------
def coupler_for(nz, micro):
    """A coupler with the five fields Kessler needs, without a dycore."""
    from miniweatherml_amd.coupler import Coupler
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(nz, NY, NX, 1)
    c.set_grid(500.0 * NX, 500.0 * NY, 20000.)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry", "temp"):
        dm.register_and_allocate(name, name, (nz, NY, NX, 1), ["z", "y", "x", "nens"])
    micro.init(c)
    return c


@pytest.mark.parametrize("sequence", [("heavy", "light", "heavy", "light"), ("light", "rejected", "heavy", "light")], ids=lambda s: "-".join(s))
def test_minimum_words_alternate_over_calls_of_unequal_weight(mw, oracle, sequence):
    """One Microphysics_Kessler, one workspace, one evolving state.  Call n accumulates its minimum in word n & 1 and resets the other
    for call n + 1: a light call behind a heavy one must not inherit the heavy call's minimum (it would sub-cycle), and a call that is
    refused before its CFL pass must not flip the parity (the word of the call after it would never have been reset).  The oracle is
    advanced in step; heavy = 0.1 s per metre of dz, light = the dycore's CFL step."""
    import torch
    from miniweatherml_amd import modules
    nz = 21
    st = edge_state(oracle, nz, HEAVY)
    micro = modules.Microphysics_Kessler()
    c = coupler_for(nz, micro)
    assert abs(c.get_dz() - st["dz"]) <= 1e-12 * st["dz"]
    dm = c.get_data_manager_readwrite()
    names = {"rho_d": "density_dry", "temp": "temp", "rho_v": "water_vapor", "rho_c": "cloud_liquid", "rho_r": "precip_liquid"}
    for k, n in names.items():
        dm.get(n).copy_(torch.from_numpy(np.array(st[k])).reshape(nz, NY, NX, 1))
    cur = {k: np.array(st[k]) for k in names}
    cur["dz"] = c.get_dz()
    ws_ptr = None
    counts = []
    for call, kind in enumerate(sequence):
        if kind == "rejected":
            with pytest.raises(modules.MWError, match="nonpositive dt"):
                micro.time_step(c, 0.0)
            continue
        dt = 0.1 * st["dz"] if kind == "heavy" else st["dt_cfl"]
        ref, ref_precl, ref_rs = reference(oracle, cur, dt)
        rs = micro.time_step(c, dt, return_rainsplit=True)
        counts.append((kind, rs))
        assert ws_ptr in (None, micro._ws.data_ptr())                              # one workspace: one pair of words
        ws_ptr = micro._ws.data_ptr()
        what = "kessler edges words %s call %d (%s)" % ("-".join(sequence), call, kind)
        assert rs == ref_rs, (what, rs, ref_rs)
        assert (rs == 1) if kind == "light" else (2 <= rs <= 8), (what, rs)
        got = {"temp": dm.get("temp"), "tracer0": dm.get("water_vapor"), "tracer1": dm.get("cloud_liquid"), "tracer2": dm.get("precip_liquid")}
        compare_fields({k: v.cpu().numpy().reshape(nz, NCOL) for k, v in got.items()}, ref, 1e-12, what)
        precl_close(dm.get("precl").cpu().numpy().reshape(NCOL), ref_precl, what)
        cur.update(temp=ref["temp"], rho_v=ref["tracer0"], rho_c=ref["tracer1"], rho_r=ref["tracer2"])
    print(counts)


# ---- 6. column edges with guard zones ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [1, 64, 65, 256, 257])
def test_column_edges_write_nothing_outside_their_arrays(mw, oracle, ncol):
    """The raw call on the LAST ncol columns of the state (wavefronts 4-8: cloud only, rainy and mixed), every array and the workspace
    inside a larger buffer of sentinels: the margins come back bit for bit, the interior is the oracle's."""
    import torch
    from miniweatherml_amd import capi
    L = capi.lib()
    nz, margin = 9, 320
    st = edge_state(oracle, nz)
    cols = np.arange(NCOL - ncol, NCOL)
    dt = st["dt_cfl"]
    ref, ref_precl, ref_rs = reference(oracle, st, dt, cols=cols, key=(nz, LIGHT, "cols", ncol))
    assert ref_rs == 1 and (ncol < 64 or ref_precl.max() > 0.0)

    def guarded(n, fill=None):
        big = torch.full((n + 2 * margin,), SENTINEL, dtype=torch.float64, device="cuda")
        inner = big[margin:margin + n]
        if fill is not None:
            inner.copy_(torch.from_numpy(np.ascontiguousarray(fill).ravel()))
        return big, inner

    order = ("rho_v", "rho_c", "rho_r", "rho_d", "temp")
    bufs = {k: guarded(nz * ncol, st[k][:, cols]) for k in order}
    bufs["precl"] = guarded(ncol)
    bufs["ws"] = guarded(L.mw_kessler_workspace_bytes(nz, ncol) // 8)
    rs = C.c_int(0)
    capi.check(L.mw_kessler_time_step(nz, ncol, st["dz"], float(dt), *[C.c_void_p(bufs[k][1].data_ptr()) for k in order],
                                      C.c_void_p(bufs["precl"][1].data_ptr()), C.c_void_p(bufs["ws"][1].data_ptr()), C.byref(rs), None))
    assert rs.value == ref_rs
    for k, (big, inner) in bufs.items():
        host = big.cpu().numpy()
        n = inner.numel()
        sent = np.full(margin, SENTINEL)
        assert same_bits(host[:margin], sent) and same_bits(host[margin + n:], sent), "%s: a margin was written" % k
    what = "kessler edges guard zones ncol=%d" % ncol
    got = {"temp": bufs["temp"][1], "tracer0": bufs["rho_v"][1], "tracer1": bufs["rho_c"][1], "tracer2": bufs["rho_r"][1]}
    compare_fields({k: v.cpu().numpy().reshape(nz, ncol) for k, v in got.items()}, ref, 1e-12, what)
    precl_close(bufs["precl"][1].cpu().numpy(), ref_precl, what)
    assert same_bits(bufs["rho_d"][1].cpu().numpy().reshape(nz, ncol), st["rho_d"][:, cols])


# ---- 7. the teacher at other chunk lengths -----------------------------------------------------------------------------------------------
def test_teacher_equals_kessler_alone_at_other_chunk_lengths(mw):
    """270 kernel columns (90 x 3 members, a partial second workgroup).  The teacher's chunk length comes from ncol * nens, Kessler
    alone's from ncol: its labels are Kessler's bits only if the chunk length does not matter.  The first 30 columns carry neither rain
    nor cloud in any member, so that the teacher too meets a rain-free and a mixed wavefront."""
    from test_gpu_surrogate_harvest import is_sentinel, teacher
    from test_gpu_surrogate_rollout import OUT4, kessler_alone, make_state, same
    shape = (26, 3, 30, 3)
    state = make_state(shape, seed=sum(shape))
    for n in ("cloud_liquid", "precip_liquid"):
        state[n][:, 0, :, :] = 0.0
    alone, counts = zip(*[kessler_alone(state, m, 0, return_rainsplit=True) for m in range(3)])
    assert counts == (1, 1, 1)
    try:
        for members in ([1, 2], [2, 0]):
            for ov in (8, 25, SINGLE):
                set_chunk(ov)
                outs, rs, _ = teacher(state, members)
                assert rs == [1, 1]
                for m in range(3):
                    for n, o in zip(OUT4, outs):
                        if m in members:
                            assert same(o[..., m], alone[m][n][..., 0]), (n, m, members, ov)
                        else:
                            assert is_sentinel(o[..., m]), (n, m, members, ov)
    finally:
        set_chunk(0)


# ---- 8. the override is what the sweeps run with -----------------------------------------------------------------------------------------
def test_the_override_is_what_the_sweeps_run_with(mw, oracle):
    """Everything above would pass with an override that nothing honours.  The CFL pass writes one flux_top row per chunk top, for every
    column that takes part: on a workspace of sentinels, exactly ceil(nz / chunk) - 1 rows lose them -- in mw_kessler_time_step, and in
    mw_kessler_members_teacher for the listed members' columns only."""
    import torch
    from miniweatherml_amd import capi, modules
    from test_gpu_surrogate_rollout import load, make_coupler, make_state
    L = capi.lib()
    nz = 26
    st = edge_state(oracle, nz)
    assert L.mw_kessler_chunk(nz, NCOL) == 4 and L.mw_kessler_chunk(nz, 270) == 4
    shape = (nz, 3, 30, 3)
    state = make_state(shape, seed=sum(shape))
    c = make_coupler(*shape, modules.Microphysics_Kessler())
    load(c, state)
    try:
        for ov, chunk in ((0, 4), (4, 4), (5, 5), (8, 8), (20, 20), (25, 25), (SINGLE, nz)):
            set_chunk(ov)
            rows = (nz + chunk - 1) // chunk - 1
            t = {n: torch.from_numpy(np.array(st[n])).cuda() for n in ("rho_v", "rho_c", "rho_r", "rho_d", "temp")}
            precl = torch.empty(NCOL, dtype=torch.float64, device="cuda")
            ws = torch.full((L.mw_kessler_workspace_bytes(nz, NCOL) // 8,), SENTINEL, dtype=torch.float64, device="cuda")
            rs = C.c_int(0)
            capi.check(L.mw_kessler_time_step(nz, NCOL, st["dz"], st["dt_cfl"], *[C.c_void_p(t[k].data_ptr()) for k in ("rho_v", "rho_c", "rho_r", "rho_d", "temp")],
                                              C.c_void_p(precl.data_ptr()), C.c_void_p(ws.data_ptr()), C.byref(rs), None))
            assert rs.value == 1
            top = ws[16 + 5 * nz * NCOL:].cpu().numpy().reshape(nz // 4 + 1, NCOL)
            assert not (top[:rows] == SENTINEL).any() and (top[rows:] == SENTINEL).all(), (ov, chunk)
            assert (top[:rows] > 0.0).any() or rows == 0                           # (rain fluxes, not only the zeros of the rain-free wavefronts)
            assert (ws[:16 + 5 * nz * NCOL] == SENTINEL).all()                      # one sub-cycle: the column sweep's scratch is not touched
            # the teacher
            tws = c._ws_teacher = torch.full((L.mw_kessler_members_teacher_workspace_bytes(nz, 90, 3) // 8,), SENTINEL, dtype=torch.float64, device="cuda")
            _, counts = modules.kessler_members_teacher(c, [1, 2], 1.0, 64, return_rainsplit=True)
            assert counts == [1, 1] and c._ws_teacher is tws
            top = tws[64 + nz * 270:].cpu().numpy().reshape(nz // 4 + 1, 90, 3)
            assert not (top[:rows, :, 1:] == SENTINEL).any() and (top[rows:] == SENTINEL).all() and (top[:, :, 0] == SENTINEL).all(), (ov, chunk)
    finally:
        set_chunk(0)
