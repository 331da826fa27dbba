"""Cost of a guarded committee's step on a contiguous 400 x 400 x 100 state, five models, both widths, with 0, 1 %,
10 % and 100 % of the columns flagged; the partial shares once scattered (columns drawn at random) and once as one block of columns:

  guarded   : ms per SurrogateBank.committee_guard_apply (committee out of place, flags, columns teacher, commit)
  baseline  : ms per step composed from what existed before: committee_apply out of place with its range, a copy of the four fields,
              mw_kessler_time_step on the WHOLE member, and a select by the same flags (torch.where; the flags themselves are taken
              as given, which favours the baseline)
  committee : ms per in-place committee_apply of the same build, the unguarded member's step
  flags     : ms per mw_committee_guard_flags call alone (64 B per cell read)

Thresholds are +inf (nothing flags by size) and a column is flagged by a NaN planted in its top-level temperature, which makes the share
and the place of the flagged columns exact; the share of 100 % uses thresholds of 0 on a finite state instead.  Every repetition starts
from the same state.  Median and min-max of --reps repetitions after one warm-up of each; every repetition is timed with device events
around --calls back-to-back steps.  Before anything is timed the two forms must leave the same bits where their definitions coincide:
with nothing flagged, and with everything flagged when Kessler's count on the whole member is the guarded step's.  After every guarded
repetition (the warm-up included) the device's counts must say that each of its steps flagged exactly the case's columns.

    timeout -k 10 900 python tools/surrogate_guard_timing.py --tag mi355x

Writes profiles/surrogate_guard_<tag>.json (or --out).
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from surrogate_committee_timing import models, summary, timed  # noqa: E402

NX, NY, NZ = 400, 400, 100
DZ, DT = 200.0, 1.0
N_SEL = 5
OWN = (0, 2, 3, 4)
CASES = (("share0", 0.0, None), ("share1_scattered", 0.01, "scattered"), ("share1_block", 0.01, "block"),
         ("share10_scattered", 0.10, "scattered"), ("share10_block", 0.10, "block"), ("share100", 1.0, None))


def same_bits(a, b):
    import torch
    return all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("surrogate_guard_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd._ffi import _field_ptr_array, _ptr, _stream_ptr
    L = capi.lib()
    ncol, ncells = NX * NY, NX * NY * NZ
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cells": ncells, "columns": ncol, "models": N_SEL,
           "reps": a.reps, "steps_per_repetition": a.calls, "dz": DZ, "dt": DT,
           "flagging": "thresholds +inf and a NaN in the top-level temperature of the flagged columns; share100: thresholds 0",
           "baseline": "committee_apply out of place with range + copy of four fields + mw_kessler_time_step on the whole member + torch.where "
                       "by the same flags (taken as given)"}
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    clean = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, ncol, 1), generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    start = [t.clone() for t in clean]                       # the state every repetition starts from (clean + the planted NaNs)
    state = [t.clone() for t in clean]
    guard = modules.CommitteeGuard(state[0], NZ)
    kes = [torch.empty_like(state[0]) for _ in range(4)]     # the baseline's copy of temp, vapor, cloud, rain
    precl = torch.empty(ncol, dtype=torch.float64, device="cuda:0")
    ws = torch.empty(L.mw_kessler_workspace_bytes(NZ, ncol) // 8 + 1, dtype=torch.float64, device="cuda:0")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    sel = list(range(N_SEL))

    def reset():
        for s, t in zip(state, start):
            s.copy_(t)

    for nine in (False, True):
        bank = modules.SurrogateBank(models(N_SEL, nine))

        def kessler_whole(want_count=False):
            rs = C.c_int(0)
            for v, k in zip(OWN, kes):
                k.copy_(state[v])
            capi.check(L.mw_kessler_time_step(NZ, ncol, DZ, DT, _ptr(kes[1]), _ptr(kes[2]), _ptr(kes[3]), _ptr(state[1]), _ptr(kes[0]), _ptr(precl),
                                              _ptr(ws), C.byref(rs) if want_count else None, _stream_ptr(dev)))
            return rs.value

        for name, share, how in CASES:
            for t, c in zip(start, clean):
                t.copy_(c)
            thr = (0.0,) * 4 if share == 1.0 else (math.inf,) * 4
            cols = np.zeros(0, dtype=np.int64)
            if how == "scattered":
                cols = np.sort(rng.choice(ncol, int(round(share * ncol)), replace=False))
            elif how == "block":
                cols = ncol // 3 + np.arange(int(round(share * ncol)))
            if len(cols):
                start[0][NZ - 1, torch.as_tensor(cols, device="cuda:0"), 0] = math.nan
            mask = torch.zeros((1, ncol, 1), dtype=torch.bool, device="cuda:0")

            def guarded():
                bank.committee_guard_apply(NZ, sel, 0, state, thr, 64, DZ, DT, guard)

            def baseline():
                bank.committee_apply(NZ, sel, 0, state, guard.mean4, guard.range4)
                kessler_whole()
                for v, k, m in zip(OWN, kes, guard.mean4):
                    torch.where(mask, k, m, out=state[v])

            def committee():
                bank.committee_apply(NZ, sel, 0, state, [state[v] for v in OWN])

            def flags_pass():                                                   # the flags kernel alone, on the scratch as the last step left it
                capi.check(L.mw_committee_guard_flags(NZ, ncol, 1, 0, _field_ptr_array(guard.mean4), _field_ptr_array(guard.range4),
                                                      (C.c_double * 4)(*thr), C.c_void_p(guard.flags.data_ptr()),
                                                      C.c_void_p(guard.counts.data_ptr()), _stream_ptr(dev)))

            # the flags the guarded step finds are the baseline's mask; where the two definitions coincide the bits must
            reset()
            guard.counts.zero_()
            guarded()
            (flagged, _), = guard.read(DT)[0]
            count_guarded = guard.read(DT)[1][0]
            want = ncol if share == 1.0 else len(cols)
            if flagged != want:
                sys.exit("surrogate_guard_timing: %s: %d columns flagged, %d wanted" % (name, flagged, want))
            mask.copy_(guard.flags.view(1, ncol, 1) != 0)
            after_guarded = [t.clone() for t in state]
            reset()
            count_whole = kessler_whole(want_count=True)
            reset()
            baseline()
            coincide = share == 0.0 or (share == 1.0 and count_whole == count_guarded)
            equal = same_bits(after_guarded, state)
            if coincide and not equal:
                sys.exit("surrogate_guard_timing: %s: the guarded step and the composed form leave different bits" % name)
            waves = int((mask.view(-1).to(torch.int32).view(-1, 64).sum(dim=1) > 0).sum()) if ncol % 64 == 0 else None
            gu, ba, co, flagged_per_repetition = [], [], [], []
            for fn, into in ((guarded, None), (baseline, None), (committee, None), (guarded, gu), (baseline, ba), (committee, co)) + \
                    ((guarded, gu), (baseline, ba), (committee, co)) * (a.reps - 1):
                reset()
                guard.counts.zero_()
                ms = timed(fn, a.calls)
                if fn is guarded:                                           # every step of the repetition flagged what the case says
                    (last, total), = guard.read(DT)[0]
                    if last != want or total != a.calls * want:
                        sys.exit("surrogate_guard_timing: %s: %d columns flagged in %d steps (%d in the last), %d per step wanted"
                                 % (name, total, a.calls, last, want))
                    flagged_per_repetition.append(int(total))
                if into is not None:
                    into.append(ms)
            timed(flags_pass, a.calls)
            fl = [timed(flags_pass, a.calls) for _ in range(a.reps)]
            r = {"n_in": 9 if nine else 5, "case": name, "share": share, "placement": how, "flagged_columns": int(flagged),
                 "flagged_in_every_timed_repetition": flagged_per_repetition, "flagged_wanted_per_repetition": a.calls * want,
                 "wavefronts_with_a_flagged_column": waves, "wavefronts": ncol // 64 if ncol % 64 == 0 else None,
                 "rainsplit_guarded": count_guarded, "rainsplit_whole_member": count_whole, "definitions_coincide": bool(coincide),
                 "equal_bits": bool(equal), "guarded": summary(gu), "baseline": summary(ba), "committee_in_place": summary(co), "flags_pass_alone": summary(fl)}
            r["flags_pass_share_of_measured_hbm_rate"] = round(64.0 * ncells / (r["flags_pass_alone"]["median"] * 1e-3) / 6.29e12, 4)
            r["guarded_minus_committee_ms"] = round(r["guarded"]["median"] - r["committee_in_place"]["median"], 4)
            r["one_64B_pass_at_measured_hbm_ms"] = round(64.0 * ncells / 6.29e12 * 1e3, 4)
            r["guarded_over_baseline"] = round(r["guarded"]["median"] / r["baseline"]["median"], 4)
            r["beats_baseline_by_more_than_both_spreads"] = bool(
                r["baseline"]["median"] - r["guarded"]["median"] >
                (r["guarded"]["max"] - r["guarded"]["min"]) + (r["baseline"]["max"] - r["baseline"]["min"]))
            res["n_in%d_%s" % (r["n_in"], name)] = r
            print(json.dumps(r), flush=True)
        del bank
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_guard_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
