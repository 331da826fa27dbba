"""Dense stacks as ensemble members (csrc/mw_stack_members.hip): mw_stack_group_members_apply in place on the member-
fastest layout against MlpStack.forward of each member extracted to contiguous arrays -- bit for bit, production and strict form --
against the fp64 forward by the yardstick of test_gpu_mlp_stack.py, and through Microphysics_Rollout and the rollout_surrogates driver."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_mlp_stack import features, held_to_yardstick, make_fields, make_stack, shape_bound

pytestmark = pytest.mark.gpu

S5, S9 = (5, [64, 64, 64, 64]), (9, [64, 64, 64, 64])
GROUPS = {"one5": [(5, [17], "state")], "one9": [(9, [10], "tendency")],
          "two": [(9, [17, 5], "state"), (5, [3], "tendency")],
          "three": [(9, [10], "state"), (9, [17, 5], "tendency"), (9, [3], "state")],
          "five": [(5, [17], "tendency"), (5, [3], "state"), (5, [33], "state"), (5, [16], "tendency"), (5, [5], "state")],
          "mixed": [(5, [3], "state"), (9, [17, 5], "tendency"), S5 + ("tendency",), (9, [10], "state")],
          "big": [S5 + ("state",), S9 + ("tendency",)]}
# (group, nz, ncol, nens): the 16-column tile's edges and more than one wave; one level, the four-level pass, its edges and a carried
# level across two and three passes; members beside, between and without neighbours
CASES = [("one5", 1, 1, 1), ("one5", 5, 17, 3), ("one5", 4, 65, 5), ("one9", 1, 1, 1), ("one9", 2, 15, 3), ("one9", 4, 17, 1), ("one9", 5, 65, 3),
         ("one9", 9, 17, 5), ("two", 1, 15, 3), ("two", 5, 17, 3), ("two", 9, 65, 5), ("three", 2, 17, 3), ("three", 4, 15, 5), ("three", 9, 65, 3),
         ("five", 1, 17, 5), ("five", 5, 65, 5), ("mixed", 1, 1, 5), ("mixed", 4, 17, 5), ("mixed", 5, 15, 5), ("mixed", 9, 65, 5),
         ("big", 2, 1, 3), ("big", 5, 17, 3), ("big", 9, 65, 5)]
TAIL = 24


def make_group(key):
    return [make_stack(n_in, widths, form, seed) for seed, (n_in, widths, form) in enumerate(GROUPS[key])]


def member_fields(nz, ncol, nens, seed):
    """The five (nz, ncol, nens) fields as views of device arrays with TAIL sentinel doubles behind them, and the arrays."""
    n = nz * ncol * nens
    host = make_fields(n, seed)
    flat = [torch.full((n + TAIL,), -7.5, dtype=torch.float64, device="cuda") for _ in range(5)]
    for d, h in zip(flat, host):
        d[:n] = torch.from_numpy(h)
    return [d[:n].view(nz, ncol, nens) for d in flat], flat


def forward_of_member(stack, f5, e, strict):
    """MlpStack.forward, out of place, of member e extracted to contiguous arrays: (4 tensors (nz, ncol))."""
    from miniweatherml_amd import mlp
    handle = mlp.MlpStack(stack, "cuda")
    outs = handle.forward(f5[0].shape[0], *[f[..., e].contiguous() for f in f5], strict=strict)
    torch.cuda.synchronize()
    handle.close()
    return outs


def bits(t):
    return t.contiguous().view(torch.int64)


def shuffled_members(k, nens, seed):
    """k distinct members of [0, nens) in a shuffled order (all of them when the group fills the ensemble)."""
    return [int(m) for m in np.random.default_rng(seed).permutation(nens)[:k]]


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("key,nz,ncol,nens", CASES)
def test_member_bits_are_the_forward_kernels(mw, key, nz, ncol, nens, strict):
    from miniweatherml_amd import mlp
    stacks = make_group(key)[:nens]
    members = shuffled_members(len(stacks), nens, nz + ncol)
    f5, flat = member_fields(nz, ncol, nens, ncol)
    before = [f.clone() for f in f5]
    want = [forward_of_member(s, before, e, strict) for s, e in zip(stacks, members)]
    group = mlp.MlpStackGroup(stacks, "cuda")
    group.members_apply(nz, members, f5, strict=strict)
    torch.cuda.synchronize()
    group.close()
    for w, e in zip(want, members):
        for v, i in enumerate((0, 2, 3, 4)):
            assert torch.equal(bits(f5[i][..., e]), bits(w[v])), (key, e, i)
    others = [e for e in range(nens) if e not in members]
    assert all(torch.equal(bits(f5[i][..., others]), bits(before[i][..., others])) for i in range(5)), "another member was written"
    assert torch.equal(bits(f5[1]), bits(before[1])), "density_dry was written"
    assert all(bool((d[-TAIL:] == -7.5).all()) for d in flat), "a cell behind an array was written"


@pytest.mark.parametrize("form", ["state", "tendency"])
@pytest.mark.parametrize("n_in,widths", [(5, [17]), S5, (9, [10]), (9, [17, 5])])
def test_members_against_fp64(mw, n_in, widths, form):
    """nz = 5, ncol = 17, nens = 3, the stack on every member: each member's 85 cells against the fp64 forward by the yardstick
    max|o_kernel - o_fp64| <= 4 max|o_fp32loop - o_fp64| + 2^-23 max|o_fp64|, un-scaling, base and clip to 2 ulp."""
    from miniweatherml_amd import mlp
    stack = make_stack(n_in, widths, form, len(widths))
    f5, _ = member_fields(5, 17, 3, n_in)
    host = [f.cpu().numpy() for f in f5]
    group = mlp.MlpStackGroup([stack] * 3, "cuda")
    group.members_apply(5, [2, 0, 1], f5)
    misses = []
    for e in range(3):
        X = features(stack, [h[..., e].reshape(-1) for h in host], 5)
        y = np.stack([f5[i][..., e].reshape(-1).cpu().numpy() for i in (0, 2, 3, 4)], 1)
        misses += held_to_yardstick(stack, X, y, "%d->%r %s member %d" % (n_in, widths, form, e), shape_bound(stack, [X]))[1]
    assert not misses, misses


def test_a_member_depends_on_its_stack_alone(mw):
    """A stack's member bits alone in a group and with three others; NaN weights in one stack stay in its member."""
    from miniweatherml_amd import mlp
    stacks = make_group("mixed")
    nan = stacks[2]._replace(layers=[(W * np.float32(np.nan), b) for W, b in stacks[2].layers])
    f5, _ = member_fields(5, 17, 5, 3)
    runs = []
    for group, members in (([stacks[1]], [3]), (stacks, [0, 3, 1, 4]), ([stacks[0], stacks[1], nan, stacks[3]], [0, 3, 1, 4])):
        g = [f.clone() for f in f5]
        mlp.MlpStackGroup(group, "cuda").members_apply(5, members, g)
        runs.append(g)
    alone, four, dirty = runs
    assert all(torch.equal(bits(alone[i][..., 3]), bits(four[i][..., 3])) for i in range(5))
    assert not torch.equal(bits(four[0][..., 3]), bits(f5[0][..., 3]))
    keep = [0, 2, 3, 4]
    assert all(torch.equal(bits(dirty[i][..., keep]), bits(four[i][..., keep])) for i in range(5))
    assert bool(torch.isnan(dirty[0][..., 1]).all())


def test_entry_errors(mw):
    from miniweatherml_amd import capi, mlp
    L = capi.lib()
    handles = [mlp.MlpStack(s, "cuda") for s in make_group("two")]
    hs = (C.c_void_p * 33)(*([handles[0]._h.value] * 33))
    g = C.c_void_p()
    for n, text in ((0, b"1 to 32 stacks, got 0"), (33, b"1 to 32 stacks, got 33")):
        assert L.mw_stack_group_create(C.byref(g), n, hs) != 0 and not g.value and text in L.mw_last_error()
    hs[1] = None
    assert L.mw_stack_group_create(C.byref(g), 2, hs) != 0 and b"stack 1 is a null handle" in L.mw_last_error()
    group = mlp.MlpStackGroup(handles, "cuda")
    f5, _ = member_fields(2, 3, 3, 0)
    ptrs = (C.c_void_p * 5)(*[f.data_ptr() for f in f5])

    def apply(h, members, p):
        rc = L.mw_stack_group_members_apply(h, (C.c_int * 2)(*members), 2, 3, 3, p, None)
        return rc, L.mw_last_error()

    for members, text in (([1, 1], b"member 1 is given to two stacks"), ([0, 3], b"member 3 of stack 1 is outside [0, 3)"),
                          ([-1, 0], b"member -1 of stack 0 is outside [0, 3)")):
        rc, err = apply(group._h, members, ptrs)
        assert rc != 0 and text in err, err
    rc, err = apply(None, [0, 1], ptrs)
    assert rc != 0 and b"stack_group_members_apply: null handle" in err
    ptrs[3] = None
    rc, err = apply(group._h, [0, 1], ptrs)
    assert rc != 0 and b"stack_group_members_apply: null field" in err
    with pytest.raises(capi.MWError, match="3 members for 2 stacks"):
        group.members_apply(2, [0, 1, 2], f5)


def test_rollout_steps_its_stack_members(mw):
    """One fixed model, one committee, two stacks and persistence on a 6 x 5 x 4 coupler: after one time_step each stack member is
    MlpStack.forward of that member's state before the step, and every other member is the same rollout's without stacks."""
    from test_gpu_surrogate_rollout import fields, nets, same
    from miniweatherml_amd import modules
    from miniweatherml_amd.mlp import IN5
    models, committees = [nets(5)[0], nets(5)[1]], [("both", ["model0", "model1"])]
    stacks = [("deep", make_stack(9, [17, 5], "tendency", 1)), ("wide", make_stack(5, [33], "state", 2))]
    runs = []
    for extra in ({"stacks": stacks}, {}):
        micro = modules.Microphysics_Rollout()
        micro.init = functools.partial(micro.init, models=models, persistence=True, committees=committees, **extra)
        runs.append(modules.make_supercell(6, 5, 4, 5 + len(extra.get("stacks", ())), 3000., 2500., 20000., micro=micro))
    (c7, _, m7), (c5, _, m5) = [r[:3] for r in runs]
    assert m7.member_names == ["kessler", "model0", "model1", "both", "deep", "wide", "persistence"] and m7.stack_members == [4, 5]
    before = fields(c7, IN5)
    want = [forward_of_member(s, [before[n].reshape(4, 30, 7) for n in IN5], e, 0) for (_, s), e in zip(stacks, (4, 5))]
    m7.time_step(c7, 1.0)
    m5.time_step(c5, 1.0)
    a, b = fields(c7), fields(c5)
    for w, e in zip(want, (4, 5)):
        for v, n in enumerate(("temp", "water_vapor", "cloud_liquid", "precip_liquid")):
            assert same(a[n][..., e].reshape(4, 30), w[v]), (n, e)
    for n in a:
        assert same(a[n][..., [0, 1, 2, 3, 6]], b[n]), n


def test_driver_rolls_a_stack_out(mw, tmp_path, monkeypatch):
    """rollout_surrogates with one fixed model and one stack written by write_surrogate_stack: the member order, the `stacks` entry of
    surrogate_rollout.json and finite scores of the stack's member."""
    from test_gpu_driver import write_yaml
    from test_gpu_surrogate_eval import write_models
    from miniweatherml_amd import driver, mlp
    entries, _ = write_models(tmp_path)
    stack = make_stack(9, [17, 5], "tendency", 4)
    paths = mlp.write_surrogate_stack(stack, str(tmp_path / "stack"))
    extra = "surrogate_models:\n  - {%s}\n" % ", ".join('%s: "%s"' % kv for kv in entries[0].items())
    extra += 'surrogate_stacks:\n  - {name: deep, keras_weights_txt: "%s", nn_input_scaling: "%s", nn_output_scaling: "%s"}\n' % paths
    path, _ = write_yaml(tmp_path, nens=4, nx=16, ny=12, nz=10, xlen=8000., ylen=6000., extra=extra)
    monkeypatch.chdir(tmp_path)
    coupler, _, info = driver.run("rollout_surrogates", path, max_steps=3, quiet=True)
    doc = json.load(open(os.path.join(str(tmp_path), "surrogate_rollout.json")))
    assert doc["members"] == ["kessler", entries[0]["name"], "deep", "persistence"] and coupler.get_nens() == 4
    assert len(doc["stacks"]) == 1
    s = doc["stacks"][0]
    assert (s["name"], s["member"], s["widths"], s["form"]) == ("deep", 2, [9, 17, 5, 4], "tendency")
    assert np.array_equal(np.array(s["slopes"], np.float32), stack.slopes)
    assert doc["diverged_at"]["deep"] is None
    assert np.isfinite(np.array(doc["history"][-1]["stats"], dtype=np.float64)[2]).all()
