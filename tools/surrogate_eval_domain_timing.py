"""Cost of splitting the in-loop scores by inside / outside the training box, on the 400 x 400 x 100 state, both
widths, K = 1, 8: ms per mw_surrogate_eval_domain call against ms per mw_surrogate_eval call of the same bank on the same state in the same
run (each: its kernels and the final pass; the host copy of the result is not in it).  The boxes keep about half of the cells inside.

Median and min-max of --reps repetitions after one warm-up call of each; every repetition times --calls back-to-back calls with device events.

    timeout -k 10 600 python tools/surrogate_eval_domain_timing.py --tag mi355x

Writes profiles/surrogate_eval_domain_<tag>.json (or --out).  Not a test: no threshold is set.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from surrogate_eval_timing import NX, NY, NZ, models, state, summary  # noqa: E402


def timed(fn, reps, calls):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--models", default="1,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("surrogate_eval_domain_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, modules
    dev = torch.device("cuda:0")
    ins, truth = state(dev)
    ncells = NX * NY * NZ
    si = modules.load_surrogate_weights()[4]
    w = si[:, 1] - si[:, 0]
    box = np.stack([si[:, 0] + 0.065 * w, si[:, 1] - 0.065 * w], axis=1)        # 0.87^5: half of the uniform cells inside (width 5)
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "state": [NZ, NY, NX, 1], "cells": ncells,
           "reps": a.reps, "calls_per_repetition": a.calls, "box": modules.box_json(box), "single_cell": {}, "stencil": {}}
    L = capi.lib()
    for n_in, name in ((5, "single_cell"), (9, "stencil")):
        for k in [int(x) for x in a.models.split(",")]:
            bank = modules.SurrogateBank(models(n_in, k))
            bank.set_domain(np.stack([box] * k))
            res[name]["models_per_pass"] = {"eval": bank.group, "eval_domain": bank.domain_group}
            _, cnt = bank.evaluate_domain(NZ, ins, truth)                       # warm-up (allocates the workspaces)
            bank.evaluate(NZ, ins, truth)
            fin, ftr, st = modules._field_ptr_array(ins), modules._field_ptr_array(truth), modules._stream_ptr(dev)
            pd, pdc = C.c_void_p(bank._dbuf.data_ptr()), C.c_void_p(bank._dbuf.data_ptr() + 8 * k * 128)
            pe, pec = C.c_void_p(bank._buf.data_ptr()), C.c_void_p(bank._buf.data_ptr() + 8 * (k + 1) * 32)
            split = timed(lambda: capi.check(L.mw_surrogate_eval_domain(bank._h, NZ, NX * NY, fin, ftr, pd, pdc, st)), a.reps, a.calls)
            whole = timed(lambda: capi.check(L.mw_surrogate_eval(bank._h, NZ, NX * NY, fin, ftr, pe, pec, st)), a.reps, a.calls)
            r = {"eval_domain": summary(split), "eval": summary(whole), "inside_share_of_cells_model0": float(cnt[0, 0].sum()) / ncells}
            r["eval_domain_over_eval"] = round(r["eval_domain"]["median"] / r["eval"]["median"], 4)
            res[name]["K%d" % k] = r
            print("%-11s K=%-3d %s" % (name, k, json.dumps(r)), flush=True)
            del bank
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_eval_domain_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
