"""Cost of the water fixer on a member-fastest 400 x 400 x 100 state with eight members, every member listed,
accumulated and fixed:

  surface_rain      : ms per mw_member_surface_rain, the call the fixer replaces (24 B read per cell and member)
  water_fix_0       : ms per mw_member_water_fix with no column to fix (the same 24 B, plus the block rows and the final kernel)
  water_fix_50/_100 : ... with about half / all of the columns fixed: a fixed column is read twice and written once (72 B per cell)
  step_off / step_on: ms per Microphysics_Rollout.time_step (Kessler, six single-cell models, persistence) with surface_rain, without
                      and with the fixer on the six models' members; and the share of their columns the step fixed.  The draws' output
                      biases of the three water fields are set to 0.5 (models 0 .. 2: about the state's own mean, so about half of
                      their columns gain water) and to 1.0 (models 3 .. 5: every column gains)

W_before is the state's own column water times 1.1 (no column gained), 0.9 (every column gained) or one of the two per column.  A call
that fixed columns leaves nothing to fix, so every timed call -- of all four kernels alike -- stands alone between two device events, and
the three water fields are restored before it, outside the events.  The kernels are interleaved (rain, 0, 50, 100, rain, ...), --calls
calls per repetition (their mean is the repetition's figure), --reps repetitions after one warm-up; the two steps alternate too.
Rates are against the bytes each case must move.

    timeout -k 10 900 python tools/water_fixer_timing.py --tag mi355x

Writes profiles/water_fixer_<tag>.json (or --out).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from surrogate_committee_timing import models, summary, timed  # noqa: E402

NX, NY, NZ, NENS = 400, 400, 100, 8
DT = 1.0
PEAK_TB_S = 6.29                                                    # the streaming rate DESIGN.md 13.7 measures against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("water_fixer_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    names = ["m%d" % k for k in range(NENS - 2)]
    micro = modules.Microphysics_Rollout()
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(NZ, NY, NX, NENS)
    c.set_grid(100.0 * NX, 100.0 * NY, 200.0 * NZ)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry", "temp"):
        dm.register_and_allocate(name, name, (NZ, NY, NX, NENS), ["z", "y", "x", "nens"])
    nets = models(NENS - 2, False)
    for k, net in enumerate(nets):                                         # (a fresh draw's biases are zero: it would remove all water)
        net[3][1:] = 0.5 if k < 3 else 1.0
    micro.init(c, nets, True, names)
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    order = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
    water = order[2:]
    start = {}
    for i, name in enumerate(order):
        start[name] = si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, NENS), generator=g, device="cuda:0", dtype=torch.float64)

    def reset(fields=order):
        for name in fields:
            dm.get(name).copy_(start[name])

    cells, plane = NX * NY * NZ * NENS, NX * NY * NENS
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "members": NENS,
           "cells_times_members": cells, "reps": a.reps, "calls_per_repetition": a.calls, "dt": DT, "models": "six single-cell draws, water output biases 0.5 (three) and 1.0 (three)",
           "peak_tb_per_s": PEAK_TB_S}
    reset()
    w_now = modules.member_column_water(c)
    half = torch.rand(w_now.shape, generator=g, device="cuda:0", dtype=torch.float64) < 0.5
    before = {"0": 1.1 * w_now, "50": torch.where(half, 0.9 * w_now, 1.1 * w_now).contiguous(), "100": 0.9 * w_now}
    total = torch.zeros_like(w_now)
    everyone = list(range(NENS))
    last = {}

    def rain():
        modules.member_surface_rain(c, everyone, everyone, DT, before["0"], total)

    def fix(case):
        def call():
            last[case] = modules.water_fix_finish([dm.get(n) for n in water], NZ, NY * NX, NENS, everyone, everyone, everyone, 0.0, c.get_dz(), DT,
                                                  before[case].view(-1), dm.get("precl"), total.view(-1), holder=c)
        return call

    kernels = [("surface_rain", rain, 0.0)] + [("water_fix_" + k, fix(k), float(k) / 100.0) for k in ("0", "50", "100")]
    ms = {k: [] for k, _, _ in kernels}
    fixed_share = {}
    for rep in range(a.reps + 1):
        for k, fn, _ in kernels:
            one = []
            for _ in range(a.calls):
                reset(water)
                one.append(timed(fn, 1))
            if rep:
                ms[k].append(sum(one) / len(one))
            if k != "surface_rain" and rep == 0:
                _, counts = last[k[len("water_fix_"):]].host()
                fixed_share[k] = float(counts.reshape(NENS, 2)[:, 0].sum()) / plane
    for k, _, nominal in kernels:
        share = fixed_share.get(k, 0.0)
        nbytes = (24.0 + 48.0 * share) * cells
        res[k] = dict(summary(ms[k]), bytes=nbytes, columns_fixed_share=round(share, 4))
        for q in ("median", "min", "max"):
            res[k]["tb_per_s_at_" + q] = round(nbytes / (res[k][q] * 1e-3) / 1e12, 3)
        res[k]["share_of_peak_at_median"] = round(res[k]["tb_per_s_at_median"] / PEAK_TB_S, 3)
        res[k]["over_surface_rain"] = round(res[k]["median"] / res["surface_rain"]["median"], 4)
        print(json.dumps({k: res[k]}), flush=True)

    steps = {"step_off": [], "step_on": []}
    for rep in range(a.reps + 1):
        for k, option in (("step_off", None), ("step_on", {"members": names})):
            reset()
            micro.surface_rain, micro.water_fixer = {}, option
            t = timed(lambda: micro.time_step(c, DT), 1)
            if rep:
                steps[k].append(t)
            if option is not None and rep == 0:
                micro.water_fix_record(0)
                tot = micro.water_fix_reports()["totals"]
                res["step_on_columns_fixed_share"] = round(sum(tot[n]["columns_fixed"] for n in names) / (len(names) * NX * NY), 4)
    for k in steps:
        res[k] = summary(steps[k])
    res["step_on_minus_off_ms"] = round(res["step_on"]["median"] - res["step_off"]["median"], 4)
    res["step_on_over_off"] = round(res["step_on"]["median"] / res["step_off"]["median"], 4)
    print(json.dumps({k: res[k] for k in ("step_off", "step_on", "step_on_minus_off_ms", "step_on_over_off", "step_on_columns_fixed_share")}), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "water_fixer_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
