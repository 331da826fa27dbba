"""Guarded committees of dense stacks (mw_stack_group_committee_guard_flag): the fused mean, flags and count against the
numpy rule -- test_gpu_stack_committee.rule (numpy on MlpStack.forward) for mean and range, test_gpu_committee_guard.host_flags on those
for the flags --, the step against its composition from Kessler on the flagged columns alone, and the rollout.  Equal is the same bits."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from committee_ref import same_bits
from test_gpu_committee_guard import DZ, gpu, host_flags, ix, kessler_on, member_state
from test_gpu_mlp_stack import make_stack
from test_gpu_stack_committee import OWN, rule, stacks_of, tailed_like
from test_gpu_stack_members import TAIL, bits, member_fields

pytestmark = pytest.mark.gpu


def thresholds(want, chosen):
    """thr[f]: the largest range of field f in column `chosen` of the reference, exactly -- that column is not flagged by f, a column with
    a larger range is; cloud_liquid never flags by size."""
    thr = [float(want[v][1][:, chosen].max()) for v in range(4)]
    thr[2] = math.inf
    return thr


def fused_against_the_rule(stacks, sel, shape, strict, seed):
    """One committee, one state: the call with and without range4, twice each."""
    from miniweatherml_amd import mlp
    nz, ncol, nens = shape
    e = (nz + ncol) % nens
    f5, flat5 = member_fields(nz, ncol, nens, seed)
    chosen, nan_col = ncol // 3, (ncol - 1 if ncol > 1 else None)
    if nan_col is not None:
        f5[0][nz - 1, nan_col, e] = math.nan                                   # the top-level temp of another column: its mean is NaN
    before = [d.clone() for d in flat5]
    want = rule([stacks[j] for j in sel], f5, e, strict)
    thr = thresholds(want, chosen)
    flagged = host_flags([w[0] for w in want], [w[1] for w in want], thr)
    assert not flagged[chosen] and (nan_col is None or flagged[nan_col])
    assert ncol < 17 or 0 < flagged.sum() < ncol
    n = int(flagged.sum())
    group = mlp.MlpStackGroup(stacks, "cuda")
    group.strict = strict
    for with_range in (1, 0):
        outs = [tailed_like(f5[0]) for _ in range(8)]
        flags = torch.full((ncol + TAIL, nens), 7, dtype=torch.uint8, device="cuda")
        counts = gpu(np.array([99, 5], dtype=np.int64))
        guard = types.SimpleNamespace(mean4=[o[0] for o in outs[:4]], range4=[o[0] for o in outs[4:]] if with_range else None, flags=flags,
                                      counts=counts.view(1, 2), check_layout=lambda *a: None, flagged_members=set())
        for calls in (1, 2):
            group.committee_guard_flag(nz, sel, e, f5, thr, guard)
            torch.cuda.synchronize()
            assert counts.cpu().tolist() == [n, 5 + calls * n], (with_range, calls)
            for v in range(4):
                assert same_bits(guard.mean4[v][..., e].cpu().numpy(), want[v][0]), ("mean", v, with_range)
                assert not with_range or same_bits(guard.range4[v][..., e].cpu().numpy(), want[v][1]), ("range", v)
            got = flags.cpu().numpy()
            assert np.array_equal(got[:ncol, e], flagged.astype(np.uint8)), np.nonzero(got[:ncol, e] != flagged)[0]
            assert (np.delete(got[:ncol], e, axis=1) == 7).all() and (got[ncol:] == 7).all(), "a flag byte of another member or behind the array was written"
        others = [m for m in range(nens) if m != e]
        for o, flat in outs:
            assert bool((o[..., others] == -7.5).all()) and bool((flat[-TAIL:] == -7.5).all()), "another member or a tail of an output was written"
        assert with_range or all(bool((o == -7.5).all()) for o, _ in outs[4:])
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat5, before)), "an input was written"
    group.close()


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 17, 3), (9, 65, 3)])
@pytest.mark.parametrize("key", ["one", "three5", "three9", "chunked"])
def test_fused_call_is_the_numpy_rule(mw, key, shape, strict):
    """nz no multiple of the four tiles, a partial column tile, a fifth tile on a second wave, an interleaved member; `chunked` is two
    k_stack_committee launches and the guard kernel reading their workspace."""
    stacks = stacks_of(key)
    fused_against_the_rule(stacks, list(range(len(stacks))), shape, strict, shape[1])


@pytest.mark.parametrize("n_in", [5, 9])
def test_a_wave_makes_a_second_grid_stride_pass(mw, n_in):
    """1024 workgroups of four waves of 16 columns: column 65,536 is wave 0's second pass, in the column walk of either width."""
    stacks = [make_stack(n_in, [3], "state", 1), make_stack(n_in, [5], "tendency", 2)]
    fused_against_the_rule(stacks, [1, 0], (2, 65537, 2), 0, n_in)


@pytest.mark.parametrize("nens,member", [(1, 0), (4, 2)])
@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("n_in", [5, 9])
def test_the_step_is_its_composition(mw, n_in, strict, nens, member):
    from miniweatherml_amd import mlp, modules
    nz, ncol, dt = 8, 65, 1.0
    stacks = stacks_of("three%d" % n_in)
    sel = [2, 0, 1]
    f5 = [gpu(a) for a in member_state(nz, ncol, nens, seed=n_in + nens)]
    want = rule([stacks[j] for j in sel], f5, member, strict)
    col_max = want[0][1].max(axis=0)
    assert (want[0][1] != 0).any(axis=0).all() and np.isfinite(col_max).all()      # a threshold of 0 flags every column
    group = mlp.MlpStackGroup(stacks, "cuda")
    group.strict = strict
    plain = [t.clone() for t in f5]
    group.committee_apply(nz, sel, member, plain, [plain[v] for v in OWN])
    kes, count = kessler_on(f5, np.arange(ncol), member, dt)
    for kind, thr4 in (("none", (math.inf,) * 4), ("all", (0.0,) * 4), ("some", (float(np.median(col_max)), math.inf, math.inf, math.inf))):
        flagged = host_flags([w[0] for w in want], [w[1] for w in want], thr4)
        F = np.nonzero(flagged)[0]
        assert len(F) == {"none": 0, "all": ncol}.get(kind, len(F)) and (kind != "some" or 0 < len(F) < ncol)
        part, pcount = kessler_on(f5, F, member, dt) if len(F) else (None, 1)
        expect = [t.clone() for t in f5]
        for at, v in enumerate(OWN):                                            # host flags, Kessler on those columns alone, the mean elsewhere
            mean = gpu(want[at][0])
            expect[v][..., member] = torch.where(gpu(flagged)[None, :], mean.index_copy(1, ix(F), part[at]) if len(F) else mean, mean)
        state = [t.clone() for t in f5]
        g = modules.CommitteeGuard(state[0], nz, ranges=False)
        group.committee_guard_apply(nz, sel, member, state, thr4, 64, DZ, dt, g)
        assert g.range4 is None and g.read(dt, [member]) == ([(len(F), len(F))], [pcount]), kind
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(state, expect)), kind
        if kind == "none":
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(state, plain))
        elif kind == "all":
            assert pcount == count and all(torch.equal(bits(state[v][..., member]), bits(k)) for v, k in zip(OWN, kes))
    group.close()


def test_rollout_with_a_range_guarded_committee(mw):
    """Kessler, the committee, its guarded twin (from one state), the two stacks, persistence on a 13 x 9 x 9 state.  Thresholds of +inf:
    the twin keeps the unguarded committee's bits over three steps.  Thresholds of 0: every column goes to Kessler at every scoring step."""
    from test_gpu_surrogate_rollout import fields, load, make_coupler, make_state
    from miniweatherml_amd import modules
    stacks = [("deep", make_stack(5, [17, 5], "tendency", 1)), ("wide", make_stack(5, [33], "state", 2))]
    state = make_state((13, 9, 9, 6), seed=23)
    for a in state.values():
        a[..., 2] = a[..., 1]
    for thr in (math.inf, 0.0):
        micro = modules.Microphysics_Rollout()
        c = make_coupler(13, 9, 9, 6, micro, models=[], persistence=True, stacks=stacks, committees=[
            ("plain", ["wide", "deep"]), ("guarded", ["wide", "deep"], {"temp": thr, "precip_liquid": thr, "max_rainsplit": 32})])
        assert micro.member_names == ["kessler", "plain", "guarded", "deep", "wide", "persistence"]
        load(c, state)
        for step in range(3):
            micro.time_step(c, 1.0)
            micro.guard_record(step, 1.0)
            assert thr == 0.0 or all(torch.equal(bits(t[..., 2]), bits(t[..., 1])) for t in fields(c).values())
        g = micro.guard_reports()[1]
        assert micro._guard.range4 is None and g["columns"] == 9 * 9 and g["max_rainsplit"] == 32
        assert [s["flagged"] for s in g["steps"]] == [0 if thr else 9 * 9] * 3
    with pytest.raises(modules.MWError, match="'guarded'.*its guard has a domain"):
        make_coupler(13, 9, 9, 5, modules.Microphysics_Rollout(), models=[], persistence=True, stacks=stacks,
                     committees=[("guarded", ["wide", "deep"], {"domain": True})])


def test_a_short_workspace_is_refused(mw):
    from miniweatherml_amd import capi, mlp
    group = mlp.MlpStackGroup(stacks_of("chunked"), "cuda")
    f5, _ = member_fields(2, 3, 2, 0)
    out = [torch.zeros_like(f5[0]) for _ in range(4)]
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    flags, counts = torch.zeros(6, dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = capi.lib().mw_stack_group_committee_guard_flag(group._h, 5, (C.c_int * 5)(0, 1, 2, 3, 4), 0, 2, 3, 2, ptr(f5), ptr(out), None, (C.c_double * 4)(1, 1, 1, 1),
                                                        C.c_void_p(flags.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(out[0].data_ptr()), 575, None)
    assert rc != 0 and b"needs a workspace of 576 bytes, got 575" in capi.lib().mw_last_error()
    group.close()
