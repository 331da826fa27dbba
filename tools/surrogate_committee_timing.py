"""Cost of a committee of n surrogates on a contiguous 400 x 400 x 100 state, both widths, n = 2, 5, 10, 16:

  committee : ms per mw_surrogate_committee_apply call (mean and range written out of place: 5 fields read, 8 written, whatever n is)
  baseline  : ms per n calls of the existing forward (mw_mlp_forward / mw_mlp_stencil_forward) on the same build and state, each into the
              same four temporaries.  A LOWER BOUND of any composed form: the averaging pass and the spread are left out.

Median and min-max of --reps repetitions after one warm-up of each; every repetition is timed with device events around --calls
back-to-back calls.  Before anything is timed the committee must equal the host mean (and range) of those forwards, bit for bit.

    timeout -k 10 600 python tools/surrogate_committee_timing.py --tag mi355x

Writes profiles/surrogate_committee_<tag>.json (or --out).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY, NZ = 400, 400, 100
HBM_MEASURED_TB_S = 6.29                     # MI355X, float4 copy


def summary(v):
    return {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def models(k, nine):
    """k fresh draws of one width with the shipped scaling tables."""
    import numpy as np
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    si9 = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]]))
    out = []
    for i in range(k):
        p = st.split_weights(st.initial_weights(i, 1, stencil=nine)[0])
        out.append((np.ascontiguousarray(p[0]), p[1].copy(), np.ascontiguousarray(p[2]), p[3].copy(), si9 if nine else si, so))
    return out


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def host_combine(ys):
    """The combination rule on the host: the sum in order, a true division, NaN-propagating extrema (finite values here)."""
    import numpy as np
    s, hi, lo = ys[0].copy(), ys[0].copy(), ys[0].copy()
    for y in ys[1:]:
        s = s + y
        hi, lo = np.maximum(hi, y), np.minimum(lo, y)
    return s / float(len(ys)), hi - lo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sizes", default="2,5,10,16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("surrogate_committee_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import modules
    ncells = NX * NY * NZ
    sizes = [int(x) for x in a.sizes.split(",")]
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cells": ncells, "reps": a.reps,
           "calls_per_repetition": a.calls, "hbm_measured_TB_per_s": HBM_MEASURED_TB_S,
           "bytes_per_cell": {"committee_with_range": 104, "committee_mean_only": 72, "baseline_per_model": 72},
           "baseline": "n calls of the existing forward into the same four temporaries; no averaging pass (a lower bound of a composed form)"}
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    ins = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY * NX, 1), generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    flat = [t.view(NZ, -1) for t in ins]
    outs = [torch.empty_like(ins[0]) for _ in range(4)]
    rngs = [torch.empty_like(ins[0]) for _ in range(4)]
    tmp = [torch.empty_like(flat[0]) for _ in range(4)]
    for nine in (False, True):
        nets = models(max(sizes), nine)
        bank = modules.SurrogateBank(nets)
        fwd = (lambda net: modules.mlp_stencil_forward(NZ, *flat, *net, outs=tmp)) if nine else (lambda net: modules.mlp_forward(*flat, *net, outs=tmp))
        for n in sizes:
            sel = list(range(n))
            # the committee is the host mean of the forwards (one field at a time on the host: 16 M doubles each)
            bank.committee_apply(NZ, sel, 0, ins, outs, rngs)
            same = True
            for v in range(4):
                ys = []
                for net in nets[:n]:
                    fwd(net)
                    ys.append(tmp[v].cpu().numpy())
                mean, rng = host_combine(ys)
                same = same and np.array_equal(outs[v].cpu().numpy().reshape(mean.shape).view(np.int64), mean.view(np.int64)) \
                    and np.array_equal(rngs[v].cpu().numpy().reshape(rng.shape), rng)
                del ys
            if not same:
                sys.exit("surrogate_committee_timing: the committee of %d %s models is not the host mean of the forwards"
                         % (n, "stencil" if nine else "single-cell"))

            def baseline():
                for net in nets[:n]:
                    fwd(net)
            com, com_mean, base = [], [], []
            for _ in range(a.reps):
                com.append(timed(lambda: bank.committee_apply(NZ, sel, 0, ins, outs, rngs), a.calls))
                com_mean.append(timed(lambda: bank.committee_apply(NZ, sel, 0, ins, outs), a.calls))
                base.append(timed(baseline, a.calls))
            r = {"n_in": 9 if nine else 5, "n": n, "committee_equals_host_mean_of_forwards": bool(same),
                 "committee": summary(com), "committee_mean_only": summary(com_mean), "baseline_n_forwards": summary(base)}
            r["committee_over_baseline"] = round(r["committee"]["median"] / r["baseline_n_forwards"]["median"], 4)
            r["beats_baseline_by_more_than_both_spreads"] = bool(
                r["baseline_n_forwards"]["median"] - r["committee"]["median"] >
                (r["committee"]["max"] - r["committee"]["min"]) + (r["baseline_n_forwards"]["max"] - r["baseline_n_forwards"]["min"]))
            r["committee_share_of_measured_hbm_rate"] = round(104.0 * ncells / (r["committee"]["median"] * 1e-3) / (HBM_MEASURED_TB_S * 1e12), 4)
            res["n_in%d_n%d" % (r["n_in"], n)] = r
            print(json.dumps(r), flush=True)
        del bank
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_committee_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
