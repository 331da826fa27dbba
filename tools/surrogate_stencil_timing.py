"""The two measurements of the stencil surrogate, stencil against single cell in ONE process on the same GPU:

  forward : cells/s of mw_mlp_stencil_forward and of mw_mlp_forward on the same 400 x 400 x 100 state (device events around --calls
            back-to-back calls, warm-up excluded, --reps repetitions, the two kernels alternating), and the bytes per cell each must move
            (9 fp64 fields: 5 in, 4 out = 72 B for both, if every input is loaded once).
  trainer : ms per epoch at the notebook's size (9,118,906 samples, batch 1024) of the stencil trainer and of the single-cell trainer,
            K = 1, 8, 64, with tools/surrogate_train_timing.py's epoch (training launch + copy + validation pass + synchronise).

    timeout -k 10 900 python tools/surrogate_stencil_timing.py --tag <tag> [--reps 3] [--only forward|trainer]
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR/fetch -- python tools/surrogate_stencil_timing.py --counter-run
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR/write -- python tools/surrogate_stencil_timing.py --counter-run
        (counters in runs of their own, ONE counter per pass: the two together exceed what the device collects at once; two calls of
         each forward, nothing timed; --counters DIR then adds the per-cell figures of those runs to the JSON)

Writes profiles/surrogate_stencil_<tag>.json (or --out).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NX, NY, NZ = 400, 400, 100


def summary(v, unit):
    return {unit: [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "spread_pct": round(100.0 * (max(v) - min(v)) / statistics.median(v), 2)}


def forward_state(dev):
    """A (nz, ny, nx, 1) state with values inside the shipped scaling ranges, and the two networks (the stencil one: the shipped rows plus
    four live level-above rows)."""
    import numpy as np
    import torch
    from miniweatherml_amd import modules
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    g = torch.Generator(device=dev).manual_seed(0)
    fields = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, 1), generator=g, device=dev, dtype=torch.float64) for i in range(5)]
    W9 = np.ascontiguousarray(np.concatenate([W1, 0.5 * W1[[0, 2, 3, 4]]]).astype(np.float32))
    si9 = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]]))
    return fields, (W1, b1, W2, b2, si, so), (W9, b1, W2, b2, si9, so)


def run_forward(a):
    import torch
    from miniweatherml_amd import modules
    dev = torch.device("cuda:0")
    fields, net5, net9 = forward_state(dev)
    outs = [torch.empty_like(fields[0]) for _ in range(4)]
    calls = {"single_cell": lambda: modules.mlp_forward(*fields, *net5, outs=outs),
             "stencil": lambda: modules.mlp_stencil_forward(NZ, *fields, *net9, outs=outs)}
    if a.counter_run:
        for _ in range(2):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        return None
    ncells = NX * NY * NZ
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.calls)
    res = {"state": [NZ, NY, NX, 1], "cells": ncells, "calls_per_repetition": a.calls, "bytes_per_cell_needed": 72,
           "timing": "device events around the back-to-back calls (host launch included), 3 warm-up calls, kernels alternating"}
    for k in calls:
        s = summary(ms[k], "ms_per_call")
        s["cells_per_s"] = round(ncells / (s["median"] * 1e-3), 0)
        s["GB_per_s_at_72B_per_cell"] = round(72.0 * ncells / (s["median"] * 1e-3) / 1e9, 1)
        res[k] = s
        print("forward %-12s %s" % (k, json.dumps(s)), flush=True)
    res["stencil_over_single_cell_time"] = round(res["stencil"]["median"] / res["single_cell"]["median"], 3)
    from miniweatherml_amd import capi
    res["stencil_z_chunk"] = int(capi.lib().mw_mlp_stencil_chunk(NZ, NX * NY))
    return res


def read_counters(d):
    """Per-cell FETCH_SIZE / WRITE_SIZE (KiB counters) of the forward kernels from a rocprofv3 --pmc run of --counter-run."""
    acc, cnt = {}, {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("mw::", "")
            if not k.startswith("k_mlp"):
                continue
            acc.setdefault(k, {}).setdefault(r["Counter_Name"], 0.0)
            acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
            cnt.setdefault(k, set()).add(r["Dispatch_Id"])
    ncells = NX * NY * NZ
    return {k: {"dispatches": len(cnt[k]), **{c + "_bytes_per_cell": round(v * 1024.0 / len(cnt[k]) / ncells, 2) for c, v in acc[k].items()}}
            for k in acc}


def synthetic9(n, device, seed=0):
    """surrogate_train_timing.synthetic with four level-above columns (rain falls in from above)."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    lo = torch.tensor([200.0, 0.1, 0.0, 0.0, 0.0, 195.0, 0.0, 0.0, 0.0], device=device)
    hi = torch.tensor([300.0, 1.2, 0.02, 0.004, 0.015, 295.0, 0.018, 0.004, 0.015], device=device)
    x = lo + (hi - lo) * torch.rand((n, 9), generator=g, device=device)
    conv = 0.3 * x[:, 3] * (1.0 + torch.tanh((x[:, 0] - 250.0) / 20.0))
    y = torch.stack([x[:, 0] + 400.0 * conv, x[:, 2] + 0.2 * conv * x[:, 1], x[:, 3] - conv + 0.1 * x[:, 7],
                     0.6 * x[:, 4] + 0.4 * x[:, 8] + 0.8 * conv], dim=1)
    return x.float().contiguous(), y.float().contiguous()


def run_trainer(a):
    import torch
    from surrogate_train_timing import time_hip
    from miniweatherml_amd.surrogate_train import split_sizes
    dev = torch.device("cuda:0")
    x9, y = synthetic9(a.n, dev)
    n_split = split_sizes(a.n)
    res = {"n_samples": a.n, "n_train": n_split[0], "n_val": n_split[1], "batch": a.batch, "reps": a.reps,
           "epoch": "training launch + copy of weights and sums + validation pass, closed by a device synchronise; warm-up epoch excluded",
           "single_cell": {}, "stencil": {}}
    scl_out = torch.stack([y.min(0).values, y.max(0).values], 1).double().cpu().numpy()
    for K in [int(k) for k in a.models.split(",")]:
        for name, raw in (("single_cell", x9[:, :5].contiguous()), ("stencil", x9)):
            scl_in = torch.stack([raw.min(0).values, raw.max(0).values], 1).double().cpu().numpy()
            r = time_hip(raw, y, scl_in, scl_out, n_split, K, a.reps, a.batch)
            res[name]["K%d" % K] = r
            print("trainer %-12s K=%-3d %s" % (name, K, json.dumps(r)), flush=True)
        res.setdefault("stencil_over_single_cell", {})["K%d" % K] = round(res["stencil"]["K%d" % K]["median_ms"] /
                                                                          res["single_cell"]["K%d" % K]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--only", choices=("forward", "trainer"), default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--n", type=int, default=9118906)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--models", default="1,8,64")
    ap.add_argument("--counter-run", action="store_true")
    ap.add_argument("--counters", default=None, help="directory of a finished rocprofv3 --pmc run of --counter-run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("surrogate_stencil_timing: no GPU (a CPU run gives no timing)")
    if a.counter_run:
        run_forward(a)
        return
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if a.only != "trainer":
        res["forward"] = run_forward(a)
        if a.counters:
            res["forward"]["rocprofv3_pmc"] = read_counters(a.counters)
            print("counters", json.dumps(res["forward"]["rocprofv3_pmc"]), flush=True)
    if a.only != "forward":
        res["trainer"] = run_trainer(a)
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_stencil_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
