"""What a committee of dense stacks costs, on 400 x 400 x 100 cells (nens = 1), for committees of 2, 5 and
16 x 5 -> 32 -> 4, 5 x 9 -> 32 -> 4 and 4 x 5 -> 64 -> 64 -> 4 (two chunks):

  mean       : MlpStackGroup.committee_apply out of place, mean only
  mean+range : the same call with range4
  forwards   : n x mw_mlp_stack_forward into temporaries, in the same run -- the floor of any composed committee, which would add the
               averaging pass (and, on the member-fastest layout, an extract and an insert) on top

Every timing: one warm-up repetition, then --reps repetitions of --calls back-to-back calls between two device events, the variants
alternating inside a repetition; medians and [min, max].  A chunked committee moves, per chunk boundary, 96 B per cell out and 96 B in
through its workspace beside the 72 B (mean+range: 104 B) per cell of the state pass.

    timeout -k 10 900 python tools/stack_committee_timing.py --tag mi355x

Writes profiles/stack_committee_<tag>.json (or --out) and prints the table of section 13.22.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mlp_stack_timing import random_stack  # noqa: E402
from tendency_timing import interleaved  # noqa: E402

NX, NY, NZ = 400, 400, 100
COMMITTEES = [(5, [32], 2), (5, [32], 5), (5, [32], 16), (9, [32], 5), (5, [64, 64], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stack_committee_timing: no GPU (a CPU run gives no timing)")
    import ctypes as C
    from miniweatherml_amd import capi, mlp, modules
    ncol = NX * NY
    _, _, _, _, si, so = modules.load_surrogate_weights()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    in5 = [(si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, ncol), generator=g, device="cuda:0", dtype=torch.float64)).reshape(NZ, ncol, 1) for i in range(5)]
    out4, range4, tmp = ([torch.empty_like(in5[0]) for _ in range(4)] for _ in range(3))
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "nens": 1, "reps": a.reps,
           "calls_per_repetition": a.calls, "cases": {}}
    for n_in, widths, k in COMMITTEES:
        key = "%d x %s" % (k, " -> ".join(str(w) for w in [n_in] + widths + [4]))
        handles = [mlp.MlpStack(random_stack(n_in, widths, si, so, j), "cuda:0") for j in range(k)]
        group = mlp.MlpStackGroup(handles, "cuda:0")
        sel, nbytes = list(range(k)), C.c_longlong(0)
        capi.check(capi.lib().mw_stack_group_committee_workspace_bytes(group._h, k, (C.c_int * k)(*sel), NZ, ncol, C.byref(nbytes)))

        def mean():
            group.committee_apply(NZ, sel, 0, in5, out4)

        def mean_range():
            group.committee_apply(NZ, sel, 0, in5, out4, range4)

        def forwards():
            for h in handles:
                h.forward(NZ, *[f.view(NZ, ncol) for f in in5], outs=[t.view(NZ, ncol) for t in tmp])

        r = interleaved([("mean", mean), ("mean+range", mean_range), ("forwards", forwards)], a.reps, a.calls)
        r["workspace_bytes_per_cell"] = nbytes.value // (NZ * ncol)
        r["mean_over_forwards"] = round(r["mean"]["median"] / r["forwards"]["median"], 4)
        r["mean_range_over_forwards"] = round(r["mean+range"]["median"] / r["forwards"]["median"], 4)
        res["cases"][key] = r
        print(json.dumps({key: r}), flush=True)
        group.close()
        for h in handles:
            h.close()
    out = a.out or os.path.join(ROOT, "profiles", "stack_committee_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    cell = lambda r: "%.3f [%.3f, %.3f]" % (r["median"], r["min"], r["max"])     # noqa: E731
    print("%-22s %26s %26s %26s %8s" % ("ms per call", "mean", "mean+range", "n forwards", "mean/fw"))
    for key, r in res["cases"].items():
        print("%-22s %26s %26s %26s %8.3f" % (key, cell(r["mean"]), cell(r["mean+range"]), cell(r["forwards"]), r["mean_over_forwards"]))
    print("wrote", out)


if __name__ == "__main__":
    main()
