"""Cost of the latent-heat closure on a member-fastest 400 x 400 x 100 state with eight members, every member
diagnosed:

  surface_rain      : ms per mw_member_surface_rain, the same-run yardstick: a read-only pass of the same mapping (24 B per cell and member)
  heat_closure_0    : ms per mw_member_heat_closure with no cell closed (closed list empty): 40 B read per cell and member, plus the block
                      rows and the final kernel
  heat_closure_100  : ... with every member closed at tolerance 0 (random noise: every cell's residual is non-zero): 40 B read and 8 B
                      written per cell and member
  before_copy       : ms per mw_members_copy of temp and water_vapor of all eight members into the two scratch fields (32 B per cell)
  step_off / step_on: ms per Microphysics_Rollout.time_step (Kessler, six single-cell models, persistence) without and with the closure
                      (every member but persistence diagnosed, the six models' members closed)

A call that closed cells leaves nothing to close, so every timed call -- of all four kernels alike -- stands alone between two device
events, and temp is restored before it, outside the events.  The kernels are interleaved (rain, 0, 100, copy, rain, ...), --calls calls
per repetition (their mean is the repetition's figure), --reps repetitions after one warm-up; the two steps alternate too.  Rates are
against the bytes each case must move.

    timeout -k 10 900 python tools/heat_closure_timing.py --tag mi355x

Writes profiles/heat_closure_<tag>.json (or --out).
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
        sys.exit("heat_closure_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import microphysics, modules
    from miniweatherml_amd.coupler import Coupler
    names = ["m%d" % k for k in range(NENS - 2)]
    micro = modules.Microphysics_Rollout()
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(NZ, NY, NX, NENS)
    c.set_grid(100.0 * NX, 100.0 * NY, 200.0 * NZ)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry", "temp"):
        dm.register_and_allocate(name, name, (NZ, NY, NX, NENS), ["z", "y", "x", "nens"])
    micro.init(c, models(NENS - 2, False), True, names)
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    order = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
    start = {}
    for i, name in enumerate(order):
        start[name] = si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, NENS), generator=g, device="cuda:0", dtype=torch.float64)

    def reset(fields=order):
        for name in fields:
            dm.get(name).copy_(start[name])

    cells, plane = NX * NY * NZ * NENS, NX * NY * NENS
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "members": NENS,
           "cells_times_members": cells, "reps": a.reps, "calls_per_repetition": a.calls, "dt": DT, "models": "six single-cell draws",
           "peak_tb_per_s": PEAK_TB_S}
    reset()
    # the state before: the state itself plus noise, so that every cell has a residual
    before2 = [start["temp"] + 0.5 * torch.randn(start["temp"].shape, generator=g, device="cuda:0", dtype=torch.float64),
               start["water_vapor"] * (1.0 + 0.01 * torch.randn(start["temp"].shape, generator=g, device="cuda:0", dtype=torch.float64))]
    scratch = [torch.empty_like(start["temp"]) for _ in range(2)]
    w_before = modules.member_column_water(c)
    total = torch.zeros_like(w_before)
    everyone = list(range(NENS))
    last = {}

    def rain():
        modules.member_surface_rain(c, everyone, everyone, DT, w_before, total)

    def closure(case, closed):
        def call():
            last[case] = microphysics.heat_closure_finish(dm.get("temp"), dm.get("density_dry"), dm.get("water_vapor"), before2, NZ, NY * NX, NENS,
                                                          everyone, closed, 0.0, c.get_dz(), DT, holder=c)
        return call

    def copy():
        microphysics.members_copy(NX * NY * NZ, NENS, everyone, [dm.get("temp"), dm.get("water_vapor")], scratch)

    kernels = [("surface_rain", rain, 24.0), ("heat_closure_0", closure("heat_closure_0", []), 40.0),
               ("heat_closure_100", closure("heat_closure_100", everyone), 48.0), ("before_copy", copy, 32.0)]
    ms = {k: [] for k, _, _ in kernels}
    share = {}
    for rep in range(a.reps + 1):
        for k, fn, _ in kernels:
            one = []
            for _ in range(a.calls):
                reset(("temp",))
                one.append(timed(fn, 1))
            if rep:
                ms[k].append(sum(one) / len(one))
            if k in last and rep == 0:
                _, counts = last[k].host()
                share[k] = float(counts.reshape(NENS, 2)[:, 0].sum()) / cells
    for k, _, per_cell in kernels:
        nbytes = (40.0 + 8.0 * share[k] if k in share else per_cell) * cells
        res[k] = dict(summary(ms[k]), bytes=nbytes)
        if k in share:
            res[k]["cells_closed_share"] = round(share[k], 4)
        for q in ("median", "min", "max"):
            res[k]["tb_per_s_at_" + q] = round(nbytes / (res[k][q] * 1e-3) / 1e12, 3)
        res[k]["share_of_peak_at_median"] = round(res[k]["tb_per_s_at_median"] / PEAK_TB_S, 3)
        res[k]["over_surface_rain"] = round(res[k]["median"] / res["surface_rain"]["median"], 4)
        print(json.dumps({k: res[k]}), flush=True)

    steps = {"step_off": [], "step_on": []}
    for rep in range(a.reps + 1):
        for k, option in (("step_off", None), ("step_on", {"closed": names})):
            reset()
            micro.heat_closure = option
            t = timed(lambda: micro.time_step(c, DT), 1)
            if rep:
                steps[k].append(t)
            if option is not None and rep == 0:
                micro.heat_closure_record(0)
                tot = micro.heat_closure_reports()["totals"]
                res["step_on_cells_closed_share"] = round(sum(tot[n]["cells_closed"] for n in names) / (len(names) * NX * NY * NZ), 4)
    for k in steps:
        res[k] = summary(steps[k])
    res["step_on_minus_off_ms"] = round(res["step_on"]["median"] - res["step_off"]["median"], 4)
    res["step_on_over_off"] = round(res["step_on"]["median"] / res["step_off"]["median"], 4)
    print(json.dumps({k: res[k] for k in ("step_off", "step_on", "step_on_minus_off_ms", "step_on_over_off", "step_on_cells_closed_share")}), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "heat_closure_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
