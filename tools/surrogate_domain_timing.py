"""Cost of the training-domain pass on a 400 x 400 x 100 state, with surrogate_guard_timing.py's protocol: median
and min-max of --reps repetitions after one warm-up of each, every repetition timed with device events around --calls back-to-back
calls.

  domain_nens1        : ms per mw_member_domain call alone, nens = 1, the one member listed, report only (40 B per cell read)
  domain_nens1_slot   : the same with the member's flag bytes and count words (the guard's call)
  domain_nens8_6      : nens = 8 with six members listed (40 B per cell of the listed members are used; the lines of all eight are
                        touched, because the members are interleaved)
  flags_nens1         : ms per mw_committee_guard_flags call alone (64 B per cell read), re-measured in this run
  copy5 / copy8       : ms per plain device copy of five / eight fields of the nens = 1 state (40 / 64 B per cell read and as many
                        written): the same-run copy rate, bytes moved (read + written) per second
  guarded_<case>      : ms per SurrogateBank.committee_guard_apply of a five-model single-cell committee without and with domain_box, with
                        0 %, 1 % (one block of columns) and 100 % of the columns flagged

The state is drawn inside the models' box, so the pass finds nothing outside on the clean state.  A column is flagged as in
surrogate_guard_timing.py: thresholds +inf and a NaN planted in its top-level temperature -- which is outside every box too, so the
guarded step flags the same columns with and without the box and the two differ by the pass alone; the share of 100 % uses thresholds
of 0.  The guarded steps use the box with a margin of 1e6: the steps of a repetition run back to back, and what five freshly drawn
models leave after the first one is anywhere in their output range, not in the box of their inputs (the pass costs the same).  After
every guarded repetition the device's counts must say that each step flagged exactly the case's columns, and the pass's own counts
must equal the planted cells.

    timeout -k 10 900 python tools/surrogate_domain_timing.py --tag mi355x

Writes profiles/surrogate_domain_<tag>.json (or --out).
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

from surrogate_committee_timing import models, summary, timed  # noqa: E402

NX, NY, NZ = 400, 400, 100
DZ, DT = 200.0, 1.0
N_SEL = 5
CASES = (("share0", 0.0), ("share1_block", 0.01), ("share100", 1.0))


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
        sys.exit("surrogate_domain_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd._ffi import _field_ptr_array, _stream_ptr
    L = capi.lib()
    ncol, ncells = NX * NY, NX * NY * NZ
    dev = torch.device("cuda:0")
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cells": ncells, "columns": ncol, "models": N_SEL,
           "reps": a.reps, "calls_per_repetition": a.calls, "dz": DZ, "dt": DT,
           "flagging": "thresholds +inf and a NaN in the top-level temperature of the flagged columns; share100: thresholds 0"}

    def measure(fn):
        timed(fn, a.calls)
        return summary([timed(fn, a.calls) for _ in range(a.reps)])

    nets = models(N_SEL, False)
    box = modules.domain_box(nets)
    wide = modules.domain_box(nets, 1.0e6)
    si = nets[0][4]
    g = torch.Generator(device="cuda:0").manual_seed(0)

    def draw(nens):
        return [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, ncol, nens), generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]

    # ---- the passes alone, nens = 1 ------------------------------------------------------------------------------------------------
    clean = draw(1)
    state = [t.clone() for t in clean]
    guard = modules.CommitteeGuard(state[0], NZ)
    counts = torch.empty((1, 16), dtype=torch.int64, device=dev)
    rows = {}
    rows["domain_nens1"] = measure(lambda: modules.member_domain(NZ, state, [0], [box], counts))
    if counts.cpu().tolist() != [[0] * 16]:
        sys.exit("surrogate_domain_timing: the clean state has cells outside the box: %r" % counts.cpu().tolist())
    rows["domain_nens1_slot"] = measure(lambda: modules.member_domain(NZ, state, [0], [box], counts, guard, [0]))
    for t in guard.mean4 + guard.range4:
        t.zero_()
    thr = (C.c_double * 4)(*[math.inf] * 4)
    rows["flags_nens1"] = measure(lambda: capi.check(L.mw_committee_guard_flags(
        NZ, ncol, 1, 0, _field_ptr_array(guard.mean4), _field_ptr_array(guard.range4), thr, C.c_void_p(guard.flags.data_ptr()),
        C.c_void_p(guard.counts.data_ptr()), _stream_ptr(dev))))
    src8, dst8 = guard.mean4 + guard.range4, [torch.empty_like(state[0]) for _ in range(8)]

    def copy(n):
        for s, d in zip(src8[:n], dst8[:n]):
            d.copy_(s)
    rows["copy5"] = measure(lambda: copy(5))
    rows["copy8"] = measure(lambda: copy(8))
    del dst8
    rate = lambda nbytes, row: nbytes / (row["median"] * 1e-3)                                  # noqa: E731   bytes per second
    copy_rate = rate(2 * 64.0 * ncells, rows["copy8"])
    res["same_run_copy_rate_TB_s"] = {"copy5": round(rate(2 * 40.0 * ncells, rows["copy5"]) / 1e12, 4), "copy8": round(copy_rate / 1e12, 4)}
    res["read_rate_TB_s"] = {k: round(rate(b * ncells, rows[k]) / 1e12, 4) for k, b in (("domain_nens1", 40.0), ("domain_nens1_slot", 40.0),
                                                                                        ("flags_nens1", 64.0))}
    res["fraction_of_same_run_copy_rate"] = {k: round(v * 1e12 / copy_rate, 4) for k, v in res["read_rate_TB_s"].items()}
    res["domain_over_flags_ms"] = round(rows["domain_nens1"]["median"] / rows["flags_nens1"]["median"], 4)
    res["expected_domain_over_flags"] = round(40.0 / 64.0, 4)

    # ---- the guarded step with and without the box ---------------------------------------------------------------------------------
    bank = modules.SurrogateBank(nets)
    sel = list(range(N_SEL))
    start = [t.clone() for t in clean]
    for name, share in CASES:
        for t, c in zip(start, clean):
            t.copy_(c)
        thr4 = (0.0,) * 4 if share == 1.0 else (math.inf,) * 4
        cols = ncol // 3 + np.arange(int(round(share * ncol))) if 0.0 < share < 1.0 else np.zeros(0, dtype=np.int64)
        if len(cols):
            start[0][NZ - 1, torch.as_tensor(cols, device="cuda:0"), 0] = math.nan
        want = ncol if share == 1.0 else len(cols)
        r = {"share": share, "flagged_columns": int(want)}
        for key, b in (("without_domain", None), ("with_domain", wide)):
            def step():
                bank.committee_guard_apply(NZ, sel, 0, state, thr4, 64, DZ, DT, guard, domain_box=b)
            ms = []
            for rep in range(a.reps + 1):
                for s, t in zip(state, start):
                    s.copy_(t)
                guard.counts.zero_()
                t_ms = timed(step, a.calls)
                (last, total), = guard.read(DT)[0]
                if last != want or total != a.calls * want:
                    sys.exit("surrogate_domain_timing: %s %s: %d columns flagged in %d steps (%d in the last), %d per step wanted"
                             % (name, key, total, a.calls, last, want))
                if rep:
                    ms.append(t_ms)
            r[key] = summary(ms)
        # the pass's own counts on the start state: the planted NaNs and nothing else
        for s, t in zip(state, start):
            s.copy_(t)
        words = modules.member_domain(NZ, state, [0], [wide], counts).cpu().tolist()[0]
        if words[2] != len(cols) or words[15] != len(cols) or sum(words) != 2 * len(cols):
            sys.exit("surrogate_domain_timing: %s: the pass counted %r, %d NaN cells in as many columns wanted" % (name, words, len(cols)))
        r["with_minus_without_ms"] = round(r["with_domain"]["median"] - r["without_domain"]["median"], 4)
        r["domain_pass_alone_ms"] = rows["domain_nens1_slot"]["median"]
        rows["guarded_" + name] = r
        print(json.dumps({name: r}), flush=True)
    del bank, guard, state, start, clean, src8

    # ---- nens = 8, six members listed ----------------------------------------------------------------------------------------------
    torch.cuda.empty_cache()
    state8 = draw(8)
    members = [1, 2, 3, 5, 6, 7]
    counts8 = torch.empty((6, 16), dtype=torch.int64, device=dev)
    boxes = [box] * 6
    rows["domain_nens8_6"] = measure(lambda: modules.member_domain(NZ, state8, members, boxes, counts8))
    if counts8.cpu().tolist() != [[0] * 16] * 6:
        sys.exit("surrogate_domain_timing: the clean nens = 8 state has cells outside the box")
    res["read_rate_TB_s"]["domain_nens8_6_listed_bytes"] = round(rate(6 * 40.0 * ncells, rows["domain_nens8_6"]) / 1e12, 4)
    res["read_rate_TB_s"]["domain_nens8_6_touched_lines"] = round(rate(8 * 40.0 * ncells, rows["domain_nens8_6"]) / 1e12, 4)
    res["fraction_of_same_run_copy_rate"]["domain_nens8_6_listed_bytes"] = round(rate(6 * 40.0 * ncells, rows["domain_nens8_6"]) / copy_rate, 4)
    res["fraction_of_same_run_copy_rate"]["domain_nens8_6_touched_lines"] = round(rate(8 * 40.0 * ncells, rows["domain_nens8_6"]) / copy_rate, 4)
    res["rows"] = rows
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    print(json.dumps({k: v["median"] for k, v in rows.items() if "median" in v}), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_domain_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
