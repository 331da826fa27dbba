"""The sparse-tracer shortcuts -- the wave-uniform zero shortcut (zero_skip), the zero-row maps with their x segments (zero_rows), zeros not
stored over zeros (zero_stores), the vapour in k_xz_state (vapour_state), the stores k_xz_state leaves out for lean tiles (lean_stores) --
under every option that keeps them switched on, on a state whose cloud crosses the periodic seams and a tile seam.

One case = one grid, one option set X, the same three time steps (dt, 2.2 dt, dt: the second has three sub-cycles, so maps are rebuilt from the
slab and the previous sub-cycle's maps feed zero_stores) run three times from identical inputs:
  A  X + the shortcut defaults, zero_verify on (and, where k_xz_state<.., VAP> can run, everything it may leave out poisoned before each step);
  B  X + zero_skip = zero_rows = vapour_state = lean_stores = 0;
  C  the CPU oracle (computed once per grid, order and state, shared by the cases).
A == B bit for bit on the eight coupler fields and the tracer stage's flag bytes after every step; zero_verify counts no violation; A and B
both meet the oracle at the production tolerances (1e-11 after one step, 1e-10 after three) without the sensitivity
fallback -- when B and C agree and A does not, the failure says so; the dispatcher's path string and the launched kernel instantiations are
the ones X asks for.

The "seam" state: the supercell, its wind disturbed so that it blows both ways across the x seam and across the y seam at different levels
(u += 6 sin(2 pi (i + 1/2) / nx) sin(pi k / nz) - 4;  v += 6 sin(2 pi (j + 1/2) / ny) sin(pi k / nz) - 5 cos(pi k / nz));  cloud in single
cells -- (k, j, i) = (1, 2, 0), (nz - 2, ny - 1, nx - 1) and, where the row has a second x tile, (3, 0, 57) and (3, 0, 58) on either side of
the tile seam; rain in one small box in mid-domain.  Members of an ensemble carry different amounts, member 0 none.  With the switches at run
time (spec = 0) ALL tracers can vanish, and a vapour that is non-zero everywhere would set every segment: there the vapour is kept in a
box that straddles the x seam only ("seam_dry").

What keeps a case from passing on a state that tests nothing, asserted in every case:
  * after step 1 the ORACLE's cloud is non-zero on the far side of the x seam from either edge speck, and across the y seam likewise;
  * (one member: the maps can be read back) in every stage of the first step the segment bits of Q_s are neither all set nor all clear over
    the rows; on rows of three tiles some tracer wave of stage 1 is lean and some is full; the segments of the LAST x tile's own cells are
    set at the level and row of the speck in cell 0 -- the seam is in the maps, whatever way the kernels address their halo;
  * (members) member 0 stays cloud-free, the others do not.

Grids: 130 x 12 x 20 (tiles of 58 + 58 + 14 cells, segments of 5, three groups of four rows, chunk_z = chunk_f = 7 and chunk_y = 9: three
z chunks with a short last one); 70 x 13 x 11 (two tiles, a last group of ONE row for the four-row workgroups, default chunks); 40 x 12 x 10
with two members (members in one workgroup) and 30 x 12 x 10 with three (member by member)."""
import math

import numpy as np
import pytest

from util import compare_fields, gpu_fields, kernel_forms, launched_kernels, push_fields, zero_row_maps, zero_row_seg_mask

pytestmark = pytest.mark.gpu

FACTORS = (1.0, 2.2, 1.0)                                        # time steps in units of the CFL step
GRIDS = {"130x12x20": (130, 12, 20, 1), "70x13x11": (70, 13, 11, 1), "40x12x10x2": (40, 12, 10, 2), "30x12x10x3": (30, 12, 10, 3)}
CHUNKS = {"130x12x20": {"chunk_z": 7, "chunk_f": 7, "chunk_y": 9}}
SHORTCUTS_OFF = {"zero_skip": 0, "zero_rows": 0, "vapour_state": 0, "lean_stores": 0}


# ------------------------------------------------------------------------------------------------------------------
# the state
# ------------------------------------------------------------------------------------------------------------------
def _specks(nx, ny, nz):
    return [(1, 2, 0), (nz - 2, ny - 1, nx - 1)] + ([(3, 0, 57), (3, 0, 58)] if nx > 58 else [])


def _seed(of, state):
    """of: the oracle's Fields of the supercell initial state, changed in place"""
    rho = of.rho_d
    nz, ny, nx, nens = rho.shape
    k = np.arange(nz, dtype=np.float64).reshape(nz, 1, 1, 1)
    j = np.arange(ny, dtype=np.float64).reshape(1, ny, 1, 1)
    i = np.arange(nx, dtype=np.float64).reshape(1, 1, nx, 1)
    of.uvel += 6.0 * np.sin(2.0 * np.pi * (i + 0.5) / nx) * np.sin(np.pi * k / nz) - 4.0
    of.vvel += 6.0 * np.sin(2.0 * np.pi * (j + 0.5) / ny) * np.sin(np.pi * k / nz) - 5.0 * np.cos(np.pi * k / nz)
    cl, pr = np.zeros(rho.shape), np.zeros(rho.shape)
    for e in range(nens):
        if nens > 1 and e == 0:
            continue                                             # member 0 of an ensemble is cloud-free
        for (kk, jj, ii) in _specks(nx, ny, nz):
            cl[kk, jj, ii, e] = 2.0e-4 * (1.0 + 0.25 * e)
        pr[nz // 2 - 1:nz // 2 + 1, ny // 2 - 1:ny // 2 + 1, nx // 2 + 3:nx // 2 + 6, e] = 1.0e-4 * (1.0 + 0.25 * e)
    of.tracers[1][...] = cl * rho
    of.tracers[2][...] = pr * rho
    if state == "seam_dry":
        of.tracers[0] *= ((k >= 4) & (k <= 7) & (j >= 4) & (j <= 7) & ((i < 5) | (i >= nx - 6))).astype(np.float64)
    else:
        assert state == "seam"


_ORACLE = {}


def _oracle_run(oracle, grid, order, state):
    """-> (the seeded initial Fields, the oracle's fields after each of the three steps, the CFL step); computed once and left unchanged"""
    key = (grid, order, state)
    if key not in _ORACLE:
        nx, ny, nz, nens = GRIDS[grid]
        O = oracle.with_order(order) if order != 5 else oracle
        odyc, of = O.supercell_setup(nx, ny, nz, nens, 500.0 * nx, 500.0 * ny, 20000.0)
        _seed(of, state)
        init = of.copy()
        dt = odyc.compute_time_step()
        steps = []
        for fac in FACTORS:
            odyc.time_step(of, dt * fac)
            steps.append({n: a.copy() for n, a in of.as_dict().items()})
        for a in [init.rho_d, init.uvel, init.vvel, init.wvel, init.temp] + init.tracers + [a for s in steps for a in s.values()]:
            a.setflags(write=False)
        _ORACLE[key] = (init, steps, dt)
    return _ORACLE[key]


def _assert_the_seams_are_crossed(c1, grid):
    """c1: the oracle's cloud after step 1"""
    nx, ny, nz, nens = GRIDS[grid]
    for e in range(1 if nens > 1 else 0, nens):
        assert c1[1, 2, nx - 1, e] != 0.0 and c1[nz - 2, ny - 1, 0, e] != 0.0, (grid, e, "x seam")
        assert c1[nz - 2, 0, nx - 1, e] != 0.0, (grid, e, "y seam, from the last row")
        if nx > 58:
            assert c1[3, ny - 1, 57, e] != 0.0 and c1[3, ny - 1, 58, e] != 0.0, (grid, e, "y seam, from row 0")
        assert float((c1[..., e] == 0.0).mean()) > 0.9, (grid, e)   # ... and the state is still sparse
    if nens > 1:
        assert not c1[..., 0].any()


# ------------------------------------------------------------------------------------------------------------------
# what the dispatcher must choose for an option set: a restatement of its rules (mw_dycore.hip: time_step; mw_march_sched.hip: rk_stage_march)
# ------------------------------------------------------------------------------------------------------------------
def _rules(grid, order, opts):
    nens = GRIDS[grid][3]
    o = {"wrap": 1, "fused_convert": 1, "fused_convert_mm": 1, "y_all": 1, "y_all_conv": 1, "mm_direct": 1, "mm_conv": 1, "spec": 1,
         "debug_vapour_redo": 0}
    o.update(opts)
    K = 1 if o["spec"] else 0
    mm_direct = nens in (2, 4) and bool(o["mm_direct"])
    layout = "nens1" if nens == 1 else "mm_direct" if mm_direct else "member_major"
    conv_in_y = bool(o["wrap"] and o["fused_convert"] and (nens == 1 or o["fused_convert_mm"]))
    # the converting first stage of a time step takes the one-launch y form unless told otherwise; a member-major handle has it for the
    # members-in-one-workgroup launches of a folded configuration only
    conv_y_all = bool(o["y_all"] and o["y_all_conv"] and (nens == 1 or (mm_direct and o["mm_conv"] and K != 0)))
    vap = bool(o["y_all"] and nens == 1 and order == 5 and K == 1)            # k_xz_state<.., VAP> behind every k_y_all (shortcuts on)
    r = {"path": "march ord%d K%d %s one_stream %s %s tracers_fused 3d" % (order, K, layout, "y_all" if o["y_all"] else "y_split",
                                                                           "conv_in_y" if conv_in_y else "conv_pass"),
         "vap": vap, "split_first": conv_in_y and not conv_y_all, "conv_in_y": conv_in_y, "y_all": bool(o["y_all"]), "mm_direct": mm_direct,
         "mm_conv": bool(o["mm_conv"]), "nens": nens, "forced_redo": bool(o["debug_vapour_redo"])}
    return r


def _vapour_stages(r, ncycles):
    """RK stages of a time step of `ncycles` sub-cycles that run the vapour form: every stage behind a k_y_all launch -- all of them, but
    for the step's first when that one converts in the split y launches"""
    if not r["vap"]:
        return 0
    return 3 * ncycles - (1 if r["split_first"] else 0)


def _assert_forms(names, r, shortcuts):
    """names: the kernels launched by handle creation and the first time step (one sub-cycle)"""
    f = kernel_forms(names)
    xz_vap = {a[7] for a in f.get("k_xz_state", ())}             # <STAGE, N1, MODE, HPL, K, ORD, MT, VAP>
    tf_vs = {a[7] for a in f.get("k_tracers_fused", ())}         # <STAGE, MODE, T, N1, K, ORD, MT, VS>
    ya_conv = {a[0] for a in f.get("k_y_all", ())}               # <CONV, K, ORD, T, MT>
    ys_conv = {a[0] for a in f.get("k_y_state", ())}             # <CONV, K, ORD, MM>
    split_y = "k_y_state" in f and "k_y_tracers" in f
    assert ("k_zero_rows" in f) == shortcuts, sorted(f)
    if shortcuts and r["vap"]:
        assert xz_vap == ({0, 1} if r["split_first"] else {1}) and tf_vs == xz_vap, (xz_vap, tf_vs)
    else:
        assert xz_vap == {0} and tf_vs == {0}, (xz_vap, tf_vs)
    if not r["y_all"]:
        assert "k_y_all" not in f and split_y and ys_conv == ({0, 1} if r["conv_in_y"] else {0})
    elif r["split_first"]:
        assert ya_conv == {0} and split_y and ys_conv == {1}, (ya_conv, ys_conv, sorted(f))   # both y forms in one step
        if r["nens"] > 1:
            assert {a[3] for a in f["k_y_state"]} == {2 if (r["mm_direct"] and r["mm_conv"]) else 1}   # (the members' converting launch)
    else:
        assert ya_conv == ({0, 1} if r["conv_in_y"] else {0}) and "k_y_state" not in f and "k_y_tracers" not in f, (ya_conv, sorted(f))
    if r["nens"] > 1:
        mt = {a[6] for a in f["k_tracers_fused"]} | {a[6] for a in f["k_xz_state"]}
        assert mt == ({0, 1} if r["mm_direct"] else {0}), mt      # members in one workgroup: the last stage's launches


# ------------------------------------------------------------------------------------------------------------------
# the runs
# ------------------------------------------------------------------------------------------------------------------
def _poison(dycore):
    from miniweatherml_amd import capi
    assert capi.lib().mw_debug_poison_handoff(dycore.h) == 0


def _assert_maps_are_mixed(maps, grid, order):
    """maps: the first step's (one sub-cycle), one member"""
    nx, ny, nz, _ = GRIDS[grid]
    every = zero_row_seg_mask(0, nx - 1, nx)
    for s in (1, 2, 3):
        seg = maps[s][:, 9:9 + ny] & np.uint32(every)
        assert (seg != 0).any() and (seg != every).any(), (grid, "stage", s)
    U = 64 - 2 * ((order - 1) // 2 + 1)                          # cells a tracer wave completes; its lanes reach U's halo and one patch cell further
    tiles = (nx + U - 1) // U
    if tiles >= 3:
        q1 = maps[1][:, 9:9 + ny]
        lean = np.stack([(q1 & np.uint32(zero_row_seg_mask(t * U - (64 - U) // 2 - 1, t * U - (64 - U) // 2 + 64, nx))) == 0 for t in range(tiles)])
        assert lean.any() and not lean.all(), grid
    # (M0: the row's own scan.  The row of the speck in cell 0 holds nothing else, and a growth that stopped at the row's end would set the
    #  segments of the cells 0 .. 9 only)
    own = zero_row_seg_mask((tiles - 1) * U, nx - 1, nx)          # the last tile's own cells, next to the seam
    assert tiles >= 2 and not (own & zero_row_seg_mask(0, 9, nx))
    assert maps[0][1, 9 + 2] & np.uint32(own), (grid, "the speck in cell 0 did not reach the last tile's segments", hex(int(maps[0][1, 9 + 2])))


def _run(grid, order, init, dt, opts, shortcuts, r):
    """-> dict(fields, flags, redo: per step; maps, kernels: of the first step; path, violations)"""
    from miniweatherml_amd import modules
    nx, ny, nz, nens = GRIDS[grid]
    coupler, dycore, _ = modules.make_supercell(nx, ny, nz, nens, 500.0 * nx, 500.0 * ny, 20000.0, ord=order)
    full = dict(opts) if shortcuts else {**opts, **SHORTCUTS_OFF}
    if shortcuts:
        full["zero_verify"] = 1
    for key, v in full.items():
        dycore.set_option(key, v)
        assert dycore.get_option(key) == v
    push_fields(coupler, init.copy())
    assert abs(dycore.compute_time_step(coupler) - dt) <= 1e-15 * dt   # (both sides take the oracle's)
    out = {"fields": [], "flags": [], "redo": [], "maps": None, "kernels": None}
    for n, fac in enumerate(FACTORS):
        if r["vap"]:
            _poison(dycore)
        dycore.time_step(coupler, dt * fac)
        out["redo"].append(dycore.vapour_redo())
        out["fields"].append(gpu_fields(coupler))
        out["flags"].append(dycore.tracer_flags().copy())
        if n == 0:
            out["maps"] = zero_row_maps(dycore)
            out["kernels"] = launched_kernels(reset=False)
    out["path"] = dycore.path()
    out["violations"] = dycore.zero_violations()
    return out


def _differences(a, b):
    """the fields (or flag bytes) of two runs: [] when they hold the same bits, else where and by how much they differ"""
    if not np.array_equal(a, b):
        d = np.argwhere(a != b)
        return ["%d cells differ, first %s, max |a - b| %.3e, a there %r, b there %r"
                % (len(d), d[:4].tolist(), float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))), a[tuple(d[0])], b[tuple(d[0])])]
    return []


def _case(oracle, grid, order, opts, state="seam"):
    nx, ny, nz, nens = GRIDS[grid]
    opts = {**({} if "chunk_model" in opts else CHUNKS.get(grid, {})), **opts}   # (forced chunk lengths would leave the chunk rule nothing to decide)
    r = _rules(grid, order, opts)
    init, ref, dt = _oracle_run(oracle, grid, order, state)
    _assert_the_seams_are_crossed(ref[0]["tracer1"], grid)
    what = "sparse options %s ord%d %s %s" % (grid, order, state, ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "default")

    A = _run(grid, order, init, dt, opts, True, r)                # first: its first step's launches are what the registry holds
    _assert_forms(A["kernels"], r, True)
    B = _run(grid, order, init, dt, opts, False, r)
    assert A["path"] == B["path"] == r["path"], (what, A["path"], B["path"], r["path"])
    assert B["maps"] is None and B["violations"][0] == -1         # (no maps, nothing verified: the shortcuts were off)
    # (from here on every finding is collected: a wrong map shows in the maps, in zero_verify's counters and in the fields, and the failure says all three)
    bad = []
    if A["violations"][0] != 0:
        bad.append("zero_verify: %d violations, by kind %r (0: the option never ran would be -1)" % A["violations"])
    if nens == 1:
        assert A["maps"] is not None, what
        try:
            _assert_maps_are_mixed(A["maps"], grid, order)
        except AssertionError as err:
            bad.append("maps of the first step: %s" % err)

    # the vapour's redo: none on this state (the vapour is smooth, as in the default run); forced: every stage that ran the vapour form
    cycles = [int(math.ceil(fac)) for fac in FACTORS]
    want = [_vapour_stages(r, n) if r["forced_redo"] else 0 for n in cycles]
    assert A["redo"] == want and B["redo"] == [0, 0, 0], (what, A["redo"], want, B["redo"])

    for n in range(len(FACTORS)):
        assert sorted(A["fields"][n]) == sorted(B["fields"][n]) == sorted(ref[n]) and len(ref[n]) == 8
        for name in sorted(ref[n]):
            assert not np.isnan(B["fields"][n][name]).any(), (what, "shortcuts off", n, name)
            bad += ["step %d %s: shortcuts on != off: %s" % (n + 1, name, m) for m in _differences(A["fields"][n][name], B["fields"][n][name])]
        bad += ["step %d flag bytes: shortcuts on != off: %s" % (n + 1, m) for m in _differences(A["flags"][n], B["flags"][n])]
    for n, tol in ((0, 1e-11), (2, 1e-10)):
        moved = []
        for side, run in (("shortcuts off", B), ("shortcuts on", A)):
            try:
                compare_fields(run["fields"][n], ref[n], tol, "%s, %s, step %d" % (what, side, n + 1))
            except AssertionError as err:
                moved.append(side)
                bad.append(str(err))
        if moved:
            bad.append("step %d: away from the oracle: %s" % (n + 1, " and ".join(moved)))
    assert not bad, "\n".join([what] + bad)

    last = A["fields"][-1]["tracer1"]
    if nens > 1:
        assert not last[..., 0].any() and all(last[..., e].any() for e in range(1, nens))
    assert float((last == 0.0).mean()) > 0.3                      # still sparse after the three steps
    return A, B


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
ONE_MEMBER = [{}, {"wrap": 0}, {"fused_convert": 0}, {"y_all_conv": 0}, {"y_all": 0}, {"tf_rows4": 0}, {"chunk_model": 0}, {"chunk_yt": 5},
              {"y_all": 0, "chunk_yt": 5},                       # (k_y_tracers is the one launch chunk_yt shapes: the split y form)
              {"wrap": 0, "tf_rows4": 0}, {"y_all_conv": 0, "debug_vapour_redo": 1}, {"wrap": 0, "debug_vapour_redo": 1}]
MEMBERS = [{}, {"wrap": 0}, {"mm_direct": 0}, {"mm_conv": 0}, {"fused_convert_mm": 0}]


def _id(opts):
    return "+".join("%s=%d" % kv for kv in opts.items()) or "default"


@pytest.mark.parametrize("opts", ONE_MEMBER, ids=_id)
@pytest.mark.parametrize("grid", ["130x12x20", "70x13x11"])
def test_one_member(mw, oracle, grid, opts):
    A, _ = _case(oracle, grid, 5, opts)
    if opts.get("y_all_conv", 1) == 0:
        # one time step launched a VAP and a non-VAP instantiation of k_xz_state, and both k_y_all and the split y kernels
        f = kernel_forms(A["kernels"])
        assert {a[7] for a in f["k_xz_state"]} == {0, 1} and {"k_y_all", "k_y_state", "k_y_tracers"} <= set(f)
        if opts.get("debug_vapour_redo"):
            assert A["redo"] == [2, 8, 2]                        # (not three per sub-cycle: the first stage of each step is split)
    elif opts.get("debug_vapour_redo"):
        assert A["redo"] == [3, 9, 3]                            # (wrap = 0 converts in a pass of its own: every stage runs the vapour form)


@pytest.mark.parametrize("grid", ["130x12x20", "70x13x11"])
def test_switches_at_run_time(mw, oracle, grid):
    """spec = 0: every tracer can vanish, the vapour too -- kept in a box on the x seam, zero elsewhere"""
    _case(oracle, grid, 5, {"spec": 0}, state="seam_dry")


@pytest.mark.parametrize("opts", [{"wrap": 0}, {"tf_rows4": 0}, {"wrap": 0, "tf_rows4": 0}], ids=_id)
@pytest.mark.parametrize("grid", ["130x12x20", "70x13x11"])
def test_weno3(mw, oracle, grid, opts):
    """WENO-3: tiles of 60 cells, two halo lanes per side"""
    _case(oracle, grid, 3, opts)


@pytest.mark.parametrize("opts", MEMBERS, ids=_id)
@pytest.mark.parametrize("grid", ["40x12x10x2", "30x12x10x3"])
def test_members(mw, oracle, grid, opts):
    """Member-major handles: one map set per member, member 0 cloud-free.  Two members: the members of a tile in one workgroup; three: one
    launch per member."""
    _case(oracle, grid, 5, opts)
