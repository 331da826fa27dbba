"""Cost of scoring K candidate surrogates in the model loop, on the 400 x 400 x 100 state, both widths, K = 1, 8, 64:

  fused    : ms per mw_surrogate_eval call (one launch of the evaluation kernel + the final pass; the host copy of the result is not in it)
  composed : the same 32 numbers per model from the entry points that existed before: once per call mw_micro_active_count with its mask;
             per model one mw_mlp_forward / mw_mlp_stencil_forward into four temporaries, then per field and class torch element-wise glue
             (d = prediction - truth masked to the class, |d|, d^2: temporaries the library has no kernel for) and one mw_mean_diff against a
             zero field for each of the three sums (24 calls per model, each a two-level sum and a host synchronise), the maxima by
             torch.amax (8 per model).  The persistence row is not in it.

Median and min-max of --reps repetitions, one warm-up call of each excluded; the fused call is timed with device events around --calls
back-to-back calls, the composed path (which synchronises the host itself) with the host clock around one pass.

    timeout -k 10 600 python tools/surrogate_eval_timing.py --tag mi355x
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/surrogate_eval_timing.py --trace-run       (a few calls of each, nothing timed)

Writes profiles/surrogate_eval_<tag>.json (or --out).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY, NZ = 400, 400, 100


def summary(v):
    return {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def state(dev):
    """Five input fields inside the shipped scaling ranges; the truth is the input on half of the cells and perturbed on the others."""
    import torch
    from miniweatherml_amd import modules
    si, so = modules.load_surrogate_weights()[4:]
    g = torch.Generator(device=dev).manual_seed(0)
    ins = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, 1), generator=g, device=dev, dtype=torch.float64) for i in range(5)]
    act = torch.rand((NZ, NY, NX, 1), generator=g, device=dev) < 0.5
    truth = [torch.where(act, ins[i] + 1e-3 * (so[v, 1] - so[v, 0]), ins[i]) for v, i in enumerate((0, 2, 3, 4))]
    return ins, truth


def models(n_in, k):
    import numpy as np
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    if n_in == 9:
        si = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]]))
    out = []
    for w in st.initial_weights(0, k, stencil=(n_in == 9)):
        p = st.split_weights(w)
        out.append((np.ascontiguousarray(p[0]), p[1].copy(), np.ascontiguousarray(p[2]), p[3].copy(), si, so))
    return out


def composed(nets, n_in, ins, truth, tmp, ws, grid, mask, zero):
    """One pass of the composed path over all models; returns (K, 2, 4, 4) lists like the fused call's rows."""
    import torch
    from miniweatherml_amd import capi, modules
    L = capi.lib()
    dev = ins[0].device
    cnt = C.c_longlong(0)
    capi.check(L.mw_micro_active_count(C.byref(grid), modules._field_ptr_array([ins[0], ins[2], ins[3], ins[4]]), modules._field_ptr_array(truth),
                                       C.c_void_p(mask.data_ptr()), C.byref(cnt), modules._stream_ptr(dev)))
    cls = [(mask == 0).reshape(ins[0].shape), (mask != 0).reshape(ins[0].shape)]
    n = ins[0].numel()
    rows = []
    for net in nets:
        if n_in == 9:
            modules.mlp_stencil_forward(NZ, *ins, *net, outs=tmp)
        else:
            modules.mlp_forward(*ins, *net, outs=tmp)
        row = []
        for c in range(2):
            row.append([])
            for p, t in zip(tmp, truth):
                d = torch.where(cls[c], p - t, zero)
                ad = d.abs()
                stats = []
                for term in (d, ad, d * d):
                    m = C.c_double(0.0)
                    capi.check(L.mw_mean_diff(n, modules._ptr(term), modules._ptr(zero), modules._ptr(ws), C.byref(m), modules._stream_ptr(dev)))
                    stats.append(m.value * n)
                stats.append(float(ad.amax()))
                row[c].append(stats)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--models", default="1,8,64")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("surrogate_eval_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, modules
    dev = torch.device("cuda:0")
    ins, truth = state(dev)
    tmp = [torch.empty_like(ins[0]) for _ in range(4)]
    ws = torch.empty(1024, dtype=torch.float64, device=dev)
    mask = torch.empty(NZ * NY * NX, dtype=torch.uint8, device=dev)
    zero = torch.zeros_like(ins[0])
    grid = capi.Grid()
    grid.nz, grid.ny, grid.nx, grid.nens = NZ, NY, NX, 1
    ncells = NX * NY * NZ
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "state": [NZ, NY, NX, 1], "cells": ncells,
           "reps": a.reps, "fused_calls_per_repetition": a.calls,
           "composed": "per call mw_micro_active_count (mask); per model: forward into 4 temporaries, torch element-wise glue for the masked "
                       "d, |d|, d^2, 24 mw_mean_diff against a zero field, 8 torch.amax: the same 32 numbers per model, no persistence row",
           "single_cell": {}, "stencil": {}}
    for n_in, name in ((5, "single_cell"), (9, "stencil")):
        for k in [int(x) for x in a.models.split(",")]:
            nets = models(n_in, k)
            bank = modules.SurrogateBank(nets)
            res[name]["models_per_pass"] = bank.group
            bank.evaluate(NZ, ins, truth)                                       # warm-up (allocates the workspace)
            rows = composed(nets[:1], n_in, ins, truth, tmp, ws, grid, mask, zero)
            got = bank.evaluate(NZ, ins, truth)[0][0]
            r0 = np.asarray(rows[0])
            res[name]["composed_vs_fused_model0_max_diff_over_max"] = float(np.max(np.abs(r0 - got)) / np.max(np.abs(got)))
            if a.trace_run:
                bank.evaluate(NZ, ins, truth)
                continue
            fused, comp = [], []
            nout = (k + 1) * 32
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    capi.check(capi.lib().mw_surrogate_eval(bank._h, NZ, NX * NY, modules._field_ptr_array(ins), modules._field_ptr_array(truth),
                                                            C.c_void_p(bank._buf.data_ptr()), C.c_void_p(bank._buf.data_ptr() + 8 * nout),
                                                            modules._stream_ptr(dev)))
                e1.record()
                torch.cuda.synchronize()
                fused.append(e0.elapsed_time(e1) / a.calls)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                composed(nets, n_in, ins, truth, tmp, ws, grid, mask, zero)
                torch.cuda.synchronize()
                comp.append((time.perf_counter() - t0) * 1e3)
            r = {"fused": summary(fused), "composed": summary(comp)}
            r["fused_over_composed"] = round(r["fused"]["median"] / r["composed"]["median"], 4)
            r["fused_ms_per_model"] = round(r["fused"]["median"] / k, 4)
            r["fused_GB_per_s_at_72B_per_cell_and_pass"] = round(72.0 * ncells * ((k + bank.group - 1) // bank.group) / (r["fused"]["median"] * 1e-3) / 1e9, 1)
            res[name]["K%d" % k] = r
            print("%-11s K=%-3d %s" % (name, k, json.dumps(r)), flush=True)
            del bank
    if a.trace_run:
        return
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_eval_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
