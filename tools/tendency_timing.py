"""What the tendency form costs, on 400 x 400 x 100 cells:

  state form against the parent : mw_mlp_forward, mw_mlp_stencil_forward and mw_surrogate_members_apply (six single-cell models, eight
                                  members) of THIS build against the same calls of another build of the library (--parent-lib: the parent
                                  commit's libmw_cdna4.so), interleaved.  The change is meant to cost the existing path nothing: the state
                                  form's median may exceed the parent's by no more than the parent's own run-to-run range.
  tendency against state        : the same three calls of this build with form = tendency (members_apply: a bank of six tendency models).
                                  The HBM bytes are the same; reported without a threshold.  --variant-lib: a build of this tree that brings the base to its
                                  lane group the OTHER way in the single-cell kernels (tools/build_variant.sh with
                                  -DMW_TENDENCY_ROTATE_FORWARD=0 -DMW_TENDENCY_ROTATE_APPLY=1: a load in k_mlp / k_mlp_x2, the 16-lane
                                  rotate in k_members_apply): timed as `tendency_variant` beside the others.
  --science DIR                 : one small table -- a state and a tendency model trained on the same generate_micro_data samples of a small
                                  supercell (same seeds and epochs), then evaluate_surrogates' rmse over persistence per class and field and
                                  rollout_surrogates' diverged_at and temperature rmse against the Kessler member at the last scoring step.
  --science DIR --domain-guard  : the rollout also carries a committee of ONE, the tendency model, with guard: {domain: {margin: 0.0}}
                                   beside the free tendency member, and training_domain: true: recorded are both
                                  members' temperature rmse at the last scoring step, the guarded member's flagged columns over time
                                  and both members' first_outside_step.  No threshold: whatever it shows.  --science-only skips the
                                  timings.

Every timing: one warm-up, then --reps repetitions of --calls back-to-back calls between two device events, the variants alternating
inside a repetition (parent, state, tendency, parent, ...); medians and ranges.

    timeout -k 10 900 python tools/tendency_timing.py --tag mi355x --parent-lib /path/to/parent/libmw_cdna4.so --science /tmp/tendency_science

Writes profiles/tendency_form_<tag>.json (or --out) and prints the table of section 13.9.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from surrogate_committee_timing import models, summary, timed  # noqa: E402

NX, NY, NZ, NENS, NMODELS = 400, 400, 100, 8, 6
FP, DP, VP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p
FWD = [VP] * 5 + [FP] * 4 + [DP] * 2 + [VP] * 4 + [VP]

YAML = """sim_time: 1000000000
nens   : {nens}
nx_glob: {n}
ny_glob: {n}
nz     : {nz}
xlen: {xlen}
ylen: {xlen}
zlen: 20000.
init_data: supercell
out_prefix: {prefix}
dt_gcm: 900
dt_phys: 0.
out_freq: -1
{extra}
"""


def parent_library(path):
    """Another build of the library beside this one (its own handle: the two builds' symbols do not meet), with the argument types of the
    entry points that existed before there were two forms."""
    L = C.CDLL(path)
    L.mw_mlp_forward.argtypes, L.mw_mlp_forward.restype = [C.c_longlong] + FWD, C.c_int
    L.mw_mlp_stencil_forward.argtypes, L.mw_mlp_stencil_forward.restype = [C.c_int, C.c_longlong] + FWD, C.c_int
    L.mw_surrogate_bank_create.argtypes, L.mw_surrogate_bank_create.restype = [C.POINTER(VP), C.c_int, C.c_int, FP, DP, DP], C.c_int
    L.mw_surrogate_members_apply.argtypes = [VP, C.POINTER(C.c_int), C.c_int, C.c_longlong, C.c_int, C.POINTER(VP), VP]
    L.mw_surrogate_members_apply.restype = C.c_int
    L.mw_last_error.restype = C.c_char_p
    return L


def variant_library(path):
    """A build of THIS tree with other compiler flags: the entry points of both forms."""
    L = parent_library(path)
    L.mw_mlp_forward_form.argtypes, L.mw_mlp_forward_form.restype = [C.c_int, C.c_longlong] + FWD, C.c_int
    L.mw_surrogate_bank_create_forms.argtypes = [C.POINTER(VP), C.c_int, C.c_int, FP, DP, DP, C.POINTER(C.c_int)]
    L.mw_surrogate_bank_create_forms.restype = C.c_int
    return L


def ok(L, rc):
    if rc != 0:
        sys.exit("tendency_timing: %s" % L.mw_last_error().decode())


def net_args(net):
    return [a.ctypes.data_as(FP) for a in net[:4]] + [net[4].ctypes.data_as(DP), net[5].ctypes.data_as(DP)]


def interleaved(variants, reps, calls):
    """{name: summary} of callables timed in turn inside each repetition, after one warm-up repetition."""
    ms = {k: [] for k, _ in variants}
    for rep in range(reps + 1):
        for k, fn in variants:
            t = timed(fn, calls)
            if rep:
                ms[k].append(t)
    return {k: summary(v) for k, v in ms.items()}


def verdict(res, key):
    """state form against the parent: the medians' difference beside the parent's own range."""
    if "parent" not in res[key]:
        return
    p, s = res[key]["parent"], res[key]["state"]
    res[key]["state_minus_parent_ms"] = round(s["median"] - p["median"], 4)
    res[key]["parent_range_ms"] = round(p["max"] - p["min"], 4)
    res[key]["state_within_parent_range"] = bool(s["median"] - p["median"] <= p["max"] - p["min"])


def timings(a, res):
    import numpy as np
    import torch
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd._ffi import _field_ptr_array, _stream_ptr
    dev = torch.device("cuda:0")
    L, P = capi.lib(), parent_library(a.parent_lib) if a.parent_lib else None
    R = variant_library(a.variant_lib) if a.variant_lib else None
    st = _stream_ptr(dev)
    n = NX * NY * NZ
    g = torch.Generator(device="cuda:0").manual_seed(0)
    net5, net9 = models(1, False)[0], models(1, True)[0]
    si = net5[4]
    ins = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand(n, generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    outs = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    ip, op = [VP(t.data_ptr()) for t in ins], [VP(t.data_ptr()) for t in outs]

    # the state form of this build writes the parent's bits (checked before anything is timed)
    if P is not None:
        keep = []
        for lib in (P, L):
            ok(lib, lib.mw_mlp_forward(n, *ip, *net_args(net5), *op, st))
            torch.cuda.synchronize()
            keep.append([o.clone() for o in outs])
            ok(lib, lib.mw_mlp_stencil_forward(NZ, NX * NY, *ip, *net_args(net9), *op, st))
            torch.cuda.synchronize()
            keep[-1] += [o.clone() for o in outs]
        res["state_form_writes_the_parents_bits"] = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(*keep))
        if not res["state_form_writes_the_parents_bits"]:
            sys.exit("tendency_timing: the state form of this build and the parent library write different bits")
        del keep

    v = [("parent", lambda: ok(P, P.mw_mlp_forward(n, *ip, *net_args(net5), *op, st)))] if P is not None else []
    v += [("state", lambda: ok(L, L.mw_mlp_forward_form(0, n, *ip, *net_args(net5), *op, st))),
          ("tendency", lambda: ok(L, L.mw_mlp_forward_form(1, n, *ip, *net_args(net5), *op, st)))]
    if R is not None:
        ok(L, L.mw_mlp_forward_form(1, n, *ip, *net_args(net5), *op, st))
        torch.cuda.synchronize()
        want = [o.clone() for o in outs]
        ok(R, R.mw_mlp_forward_form(1, n, *ip, *net_args(net5), *op, st))
        torch.cuda.synchronize()
        res["variant_writes_the_same_bits"] = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(want, outs))
        del want
        v.append(("tendency_variant", lambda: ok(R, R.mw_mlp_forward_form(1, n, *ip, *net_args(net5), *op, st))))
    res["mlp_forward"] = interleaved(v, a.reps, a.calls)
    v = [("parent", lambda: ok(P, P.mw_mlp_stencil_forward(NZ, NX * NY, *ip, *net_args(net9), *op, st)))] if P is not None else []
    v += [("state", lambda: ok(L, L.mw_mlp_stencil_forward_form(0, NZ, NX * NY, *ip, *net_args(net9), *op, st))),
          ("tendency", lambda: ok(L, L.mw_mlp_stencil_forward_form(1, NZ, NX * NY, *ip, *net_args(net9), *op, st)))]
    res["mlp_stencil_forward"] = interleaved(v, a.reps, a.calls)
    del outs, ins

    # members_apply: six models on members 1 .. 6 of eight, in place (timing only: the values run away, which costs nothing)
    six = models(NMODELS, False)
    fields = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY * NX, NENS), generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    f5 = _field_ptr_array(fields)
    members = (C.c_int * NMODELS)(*range(1, NMODELS + 1))
    bank_s, bank_t = modules.SurrogateBank(six), modules.SurrogateBank([m + ("tendency",) for m in six])
    v = []
    params = np.ascontiguousarray([np.concatenate([np.ravel(x) for x in m[:4]]) for m in six], dtype=np.float32)
    sin, sout = np.ascontiguousarray([m[4] for m in six]), np.ascontiguousarray([m[5] for m in six])
    if P is not None:
        h = VP()
        ok(P, P.mw_surrogate_bank_create(C.byref(h), 5, NMODELS, params.ctypes.data_as(FP), sin.ctypes.data_as(DP), sout.ctypes.data_as(DP)))
        v.append(("parent", lambda: ok(P, P.mw_surrogate_members_apply(h, members, NZ, NX * NY, NENS, f5, st))))
    v += [("state", lambda: ok(L, L.mw_surrogate_members_apply(bank_s._h, members, NZ, NX * NY, NENS, f5, st))),
          ("tendency", lambda: ok(L, L.mw_surrogate_members_apply(bank_t._h, members, NZ, NX * NY, NENS, f5, st)))]
    if R is not None:
        hr, forms = VP(), (C.c_int * NMODELS)(*([1] * NMODELS))
        ok(R, R.mw_surrogate_bank_create_forms(C.byref(hr), 5, NMODELS, params.ctypes.data_as(FP), sin.ctypes.data_as(DP), sout.ctypes.data_as(DP), forms))
        v.append(("tendency_variant", lambda: ok(R, R.mw_surrogate_members_apply(hr, members, NZ, NX * NY, NENS, f5, st))))
    res["members_apply"] = interleaved(v, a.reps, a.calls)
    for key, cells in (("mlp_forward", n), ("mlp_stencil_forward", n), ("members_apply", n * NMODELS)):
        verdict(res, key)
        r = res[key]
        r["tendency_minus_state_ms"] = round(r["tendency"]["median"] - r["state"]["median"], 4)
        r["state_range_ms"], r["tendency_range_ms"] = [round(r[k]["max"] - r[k]["min"], 4) for k in ("state", "tendency")]
        r["tb_per_s_at_72_bytes_per_cell"] = {k: round(72.0 * cells / (r[k]["median"] * 1e-3) / 1e12, 3) for k in r if isinstance(r[k], dict) and "median" in r[k]}
        print(json.dumps({key: r}), flush=True)


def science(a, res):
    """Train both forms on one sample file, score them in the loop, roll them out."""
    import numpy as np
    from miniweatherml_amd import driver, surrogate_train as st
    work = os.path.abspath(a.science)
    os.makedirs(work, exist_ok=True)
    here = os.getcwd()
    os.chdir(work)
    try:
        kw = dict(n=a.science_n, nz=a.science_nz, xlen=a.science_dx * a.science_n, prefix=os.path.join(work, "out"))
        path = os.path.join(work, "generate.yaml")
        open(path, "w").write(YAML.format(nens=1, extra="", **kw))
        _, _, info = driver.run("generate_micro_data", path, max_steps=a.science_steps, quiet=True)
        sample_file = os.path.join(work, "supercell_kessler_data_task_0.nc")
        print("tendency_timing: science: generated %d samples" % int(info["samples"]), flush=True)
        sci = {"grid": [a.science_n, a.science_n, a.science_nz], "dx": a.science_dx, "generate_steps": a.science_steps, "samples": int(info["samples"]), "epochs": a.science_epochs}
        entries = []
        for form in ("state", "tendency"):
            r = st.train_surrogate([sample_file], os.path.join(work, form), epochs=a.science_epochs, batch_size=256, seed=0, models=2, form=form)
            sci[form + "_val_loss_scaled_label_space"] = r["history"][r["best_model"]]["val_loss"][-1]
            p = r["files_written"]
            entries.append('  - {name: %s, keras_weights_txt: "%s", nn_input_scaling: "%s", nn_output_scaling: "%s"}\n' % (form, p[0], p[1], p[2]))
        print("tendency_timing: science: trained", flush=True)
        x, y, _ = st.read_samples([sample_file])
        d = st.tendencies(x, y)
        sci["share_of_samples_whose_temperature_label_is_zero"] = float(np.mean(d[:, 0] == 0.0))
        extra = "surrogate_models:\n" + "".join(entries)
        path = os.path.join(work, "evaluate.yaml")
        open(path, "w").write(YAML.format(nens=1, extra=extra, **kw))
        _, _, info = driver.run("evaluate_surrogates", path, max_steps=a.science_steps, quiet=True)
        rep = info["surrogate_report"]
        sci["evaluate_rmse_over_persistence"] = {m: {c: {f: rep[m][c][f]["rmse_over_persistence"] for f in ("temp", "water_vapor", "cloud_liquid", "precip_liquid")}
                                                     for c in ("inactive", "active")} for m in ("state", "tendency")}
        sci["evaluate_cells"] = {c: rep["state"][c]["n"] for c in ("inactive", "active")}
        print("tendency_timing: science: evaluated", flush=True)
        path = os.path.join(work, "rollout.yaml")
        boxed = "surrogate_committees:\n  - {name: tendency_boxed, members: [tendency], guard: {domain: {margin: 0.0}}}\ntraining_domain: true\n"
        open(path, "w").write(YAML.format(nens=5 if a.domain_guard else 4, extra=extra + "eval_interval: 100\n" + (boxed if a.domain_guard else ""), **kw))
        driver.run("rollout_surrogates", path, max_steps=a.science_steps, quiet=True)
        doc = json.load(open(os.path.join(work, "surrogate_rollout.json")))
        last = doc["report"][-1]
        scored = ("state", "tendency", "persistence") + (("tendency_boxed",) if a.domain_guard else ())
        sci["rollout"] = {"steps": doc["steps"], "last_scoring_step": last["step"], "diverged_at": doc["diverged_at"],
                          "temp_rmse_against_kessler": {m: last["members"][m]["fields"]["temp"]["rmse"] for m in scored}}
        if a.domain_guard:
            com = doc["committees"][0]
            free = [m for m in doc["models"] if m["name"] == "tendency"][0]["domain"]
            sci["domain_guard"] = {"box": com["guard"]["domain"]["box"], "columns": com["guard"]["columns"],
                                   "first_outside_step": {"tendency": free["first_outside_step"], "tendency_boxed": com["domain"]["first_outside_step"]},
                                   "flagged_total": com["guard"]["flagged_total"],
                                   "tendency_boxed_steps": [[s["step"], s["flagged"], s["outside_columns"], s["rainsplit"]] for s in com["guard"]["steps"]],
                                   "tendency_outside_columns": [[s["step"], s["outside_columns"]] for s in free["steps"]],
                                   "temp_rmse_over_time": {m: [[t["step"], t["members"][m]["fields"]["temp"]["rmse"]] for t in doc["report"]]
                                                           for m in ("tendency", "tendency_boxed", "persistence")}}
        res["science"] = sci
        print(json.dumps({"science": sci}), flush=True)
    finally:
        os.chdir(here)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmw_cdna4.so (without it: this build's two forms alone)")
    ap.add_argument("--variant-lib", default=None, help="a build with the other base scheme per kernel: its tendency form beside this build's")
    ap.add_argument("--science", default=None, metavar="DIR", help="also the small science table, with DIR as the working directory")
    ap.add_argument("--science-n", type=int, default=48)
    ap.add_argument("--science-dx", type=float, default=1500.0)
    ap.add_argument("--science-nz", type=int, default=32)
    ap.add_argument("--science-steps", type=int, default=4000)
    ap.add_argument("--science-epochs", type=int, default=20)
    ap.add_argument("--domain-guard", action="store_true", help="with --science: a domain-guarded committee of one beside the free tendency member")
    ap.add_argument("--science-only", action="store_true", help="with --science: skip the timings")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if (a.domain_guard or a.science_only) and not a.science:
        sys.exit("tendency_timing: --domain-guard and --science-only go with --science DIR")
    import torch
    if not torch.cuda.is_available():
        sys.exit("tendency_timing: no GPU (a CPU run gives no timing)")
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "members": NENS,
           "models": NMODELS, "reps": a.reps, "calls_per_repetition": a.calls, "parent_lib": bool(a.parent_lib)}
    if not a.science_only:
        timings(a, res)
    out = a.out or os.path.join(ROOT, "profiles", "tendency_form_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def write():
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    write()
    if a.science:
        try:
            science(a, res)
        except Exception as e:                                                  # the timings stand on their own
            res["science_error"] = "%s: %s" % (type(e).__name__, e)
            print(json.dumps({"science_error": res["science_error"]}), flush=True)
        write()
    if a.science_only:
        print("wrote", out)
        return
    cols = ("parent", "state", "tendency", "tendency_variant")
    print("%-22s" % "ms per call" + "".join(" %28s" % k for k in cols))
    for key in ("mlp_forward", "mlp_stencil_forward", "members_apply"):
        cell = lambda k: "%.4f [%.4f, %.4f]" % (res[key][k]["median"], res[key][k]["min"], res[key][k]["max"]) if k in res[key] else "-"   # noqa: E731
        print("%-22s" % key + "".join(" %28s" % cell(k) for k in cols))
    print("wrote", out)


if __name__ == "__main__":
    main()
