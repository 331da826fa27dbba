"""Cost of a guarded committee of dense stacks' step on a contiguous 400 x 400 x 100 state (nens = 1), for
committees of 4 x 9 -> 32 -> 4, 4 x 5 -> 64 -> 64 -> 4 (two chunks) and 3 x 5 -> 64 -> 64 -> 64 -> 64 -> 4 (three chunks), with 0, 10 % (one
block of columns) and 100 % of the columns flagged:

  fused     : ms per MlpStackGroup.committee_guard_apply -- mean, flags and count in the committee's last launch, then the commit
  composed  : ms per step of the same build's committee_apply out of place with its range, mw_committee_guard_flags, the same commit
  unguarded : ms per in-place committee_apply, the unguarded member's step

Thresholds are +inf and a column is flagged by a NaN planted in its top-level temperature (tools/surrogate_guard_timing.py's way: the
share and the place are exact); the share of 100 % uses thresholds of 0 on a finite state.  Every repetition starts from the same state.
One warm-up repetition of each form, then --reps repetitions of --calls back-to-back steps between two device events, the forms
alternating; medians and [min, max].  Before anything is timed the fused and the composed step must leave the same bits and counts.

    timeout -k 10 900 python tools/stack_guard_timing.py --tag mi355x

Writes profiles/stack_guard_<tag>.json (or --out) and prints the table of section 13.23.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mlp_stack_timing import random_stack  # noqa: E402
from surrogate_committee_timing import summary, timed  # noqa: E402

NX, NY, NZ = 400, 400, 100
DZ, DT = 200.0, 1.0
COMMITTEES = [(9, [32], 4), (5, [64, 64], 4), (5, [64, 64, 64, 64], 3)]
SHARES = (("share0", 0.0), ("share10_block", 0.10), ("share100", 1.0))
OWN = (0, 2, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stack_guard_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, mlp, modules
    from miniweatherml_amd._ffi import _field_ptr_array, _stream_ptr
    L, dev = capi.lib(), torch.device("cuda:0")
    ncol = NX * NY
    _, _, _, _, si, so = modules.load_surrogate_weights()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    clean = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, ncol, 1), generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    start, state = [t.clone() for t in clean], [t.clone() for t in clean]
    lean, full = modules.CommitteeGuard(state[0], NZ, ranges=False), modules.CommitteeGuard(state[0], NZ)
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "nens": 1, "reps": a.reps,
           "steps_per_repetition": a.calls, "dz": DZ, "dt": DT, "cases": {},
           "flagging": "thresholds +inf and a NaN in the top-level temperature of the flagged columns; share100: thresholds 0"}

    def reset():
        for s, t in zip(state, start):
            s.copy_(t)
        lean.counts.zero_()
        full.counts.zero_()

    for n_in, widths, k in COMMITTEES:
        key = "%d x %s" % (k, " -> ".join(str(w) for w in [n_in] + widths + [4]))
        handles = [mlp.MlpStack(random_stack(n_in, widths, si, so, j), "cuda:0") for j in range(k)]
        group = mlp.MlpStackGroup(handles, "cuda:0")
        sel, nbytes = list(range(k)), C.c_longlong(0)
        capi.check(L.mw_stack_group_committee_workspace_bytes(group._h, k, (C.c_int * k)(*sel), NZ, ncol, C.byref(nbytes)))
        for name, share in SHARES:
            for t, c in zip(start, clean):
                t.copy_(c)
            thr = (0.0,) * 4 if share == 1.0 else (math.inf,) * 4
            want = int(round(share * ncol))
            if 0.0 < share < 1.0:
                start[0][NZ - 1, ncol // 3:ncol // 3 + want, 0] = math.nan

            def fused():
                group.committee_guard_apply(NZ, sel, 0, state, thr, 64, DZ, DT, lean)

            def composed():
                group.committee_apply(NZ, sel, 0, state, full.mean4, full.range4)
                capi.check(L.mw_committee_guard_flags(NZ, ncol, 1, 0, _field_ptr_array(full.mean4), _field_ptr_array(full.range4), (C.c_double * 4)(*thr),
                                                      C.c_void_p(full.flags.data_ptr()), C.c_void_p(full.counts.data_ptr()), _stream_ptr(dev)))
                full.commit(NZ, [0], state, 64, DZ, DT)

            def unguarded():
                group.committee_apply(NZ, sel, 0, state, [state[v] for v in OWN])

            reset()
            for _ in range(a.calls):
                fused()
            after, got = [t.clone() for t in state], lean.read(DT)
            reset()
            for _ in range(a.calls):
                composed()
            if got != full.read(DT) or got[0] != [(want, a.calls * want)] or not torch.equal(lean.flags, full.flags) or \
                    not all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(after, state)):
                sys.exit("stack_guard_timing: %s %s: fused %r and composed %r differ, or do not flag %d columns per step" % (key, name, got, full.read(DT), want))
            ms = {"fused": [], "composed": [], "unguarded": []}
            for rep in range(a.reps + 1):
                for form, fn in (("fused", fused), ("composed", composed), ("unguarded", unguarded)):
                    reset()
                    t = timed(fn, a.calls)
                    if rep:
                        ms[form].append(t)
            r = {form: summary(v) for form, v in ms.items()}
            r.update(share=share, flagged_columns=want, rainsplit=got[1][0], workspace_bytes_per_cell=nbytes.value // (NZ * ncol))
            spreads = sum(r[f]["max"] - r[f]["min"] for f in ("fused", "composed"))
            r["fused_minus_composed_ms"] = round(r["fused"]["median"] - r["composed"]["median"], 4)
            r["verdict"] = "fused wins" if -r["fused_minus_composed_ms"] > spreads else "fused loses" if r["fused_minus_composed_ms"] > spreads else "within the spreads"
            res["cases"]["%s %s" % (key, name)] = r
            print(json.dumps({"%s %s" % (key, name): r}), flush=True)
        group.close()
        for h in handles:
            h.close()
    out = a.out or os.path.join(ROOT, "profiles", "stack_guard_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    cell = lambda r: "%.3f [%.3f, %.3f]" % (r["median"], r["min"], r["max"])     # noqa: E731
    print("%-52s %24s %24s %24s  %s" % ("ms per step", "fused", "composed", "unguarded", "verdict"))
    for key, r in res["cases"].items():
        print("%-52s %24s %24s %24s  %s" % (key, cell(r["fused"]), cell(r["composed"]), cell(r["unguarded"]), r["verdict"]))
    print("wrote", out)


if __name__ == "__main__":
    main()
