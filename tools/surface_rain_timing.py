"""Cost of the surface-rain diagnostic on a member-fastest 400 x 400 x 100 state with eight members:

  column_water  : ms per mw_member_column_water (24 B read per cell and member)
  surface_rain  : ms per mw_member_surface_rain with every member listed and accumulated (the same 24 B)
  divergence    : ms per mw_member_divergence of ONE 3-D field (8 B per cell and member), the yardstick: a streaming pass over the same
                  layout.  Each of the three also as TB/s of the bytes it must read.
  step_off / step_on : ms per Microphysics_Rollout.time_step (Kessler, six single-cell models, persistence) without and with the option

The kernels are timed interleaved (water, rain, divergence, water, ...), --calls back-to-back calls between two device events, --reps
repetitions after one warm-up of each; the two steps alternate too, one step per repetition, every repetition from the same state.
Before anything is timed the step with the option must leave the bits of the step without it.

    timeout -k 10 600 python tools/surface_rain_timing.py --tag mi355x

Writes profiles/surface_rain_<tag>.json (or --out).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("surface_rain_timing: no GPU (a CPU run gives no timing)")
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
    micro.init(c, models(NENS - 2, False), True, names)
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    order = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
    start = {}
    for i, name in enumerate(order):
        start[name] = si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, NENS), generator=g, device="cuda:0", dtype=torch.float64)

    def reset():
        for name in order:
            dm.get(name).copy_(start[name])

    cells = NX * NY * NZ * NENS
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "members": NENS,
           "cells_times_members": cells, "reps": a.reps, "calls_per_repetition": a.calls, "dt": DT, "models": "six single-cell draws"}
    # the option only reads the step
    reset()
    micro.surface_rain = None
    micro.time_step(c, DT)
    off = [dm.get(n).clone() for n in order]
    reset()
    micro.surface_rain = {}
    micro.time_step(c, DT)
    if not all(torch.equal(x.view(torch.int64), dm.get(n).view(torch.int64)) for x, n in zip(off, order)):
        sys.exit("surface_rain_timing: the step with the option leaves other bits than the step without it")
    del off
    res["step_with_the_option_leaves_the_same_bits"] = True

    w = modules.member_column_water(c)
    total = torch.zeros_like(w)
    everyone = list(range(NENS))

    def water():
        modules.member_column_water(c, out=w)

    def rain():
        modules.member_surface_rain(c, everyone, everyone, DT, w, total)

    from miniweatherml_amd import capi
    from miniweatherml_amd._ffi import StatsAndCounts, _field_ptr_array, _ptr, _stream_ptr
    L = capi.lib()
    n3 = NX * NY * NZ
    ws = torch.empty(L.mw_member_divergence_workspace_bytes(n3, NENS, 1) // 8 + 1, dtype=torch.float64, device="cuda:0")
    buf = StatsAndCounts(NENS * 7, NENS, "cuda:0")
    rain3 = _field_ptr_array([dm.get("precip_liquid")])

    def divergence():                                                       # (the kernels alone, as the other two: no copy to the host)
        capi.check(L.mw_member_divergence(n3, NENS, 1, rain3, _ptr(ws), buf.stats_ptr, buf.counts_ptr, _stream_ptr(torch.device("cuda:0"))))

    kernels = (("column_water", water, 24.0), ("surface_rain", rain, 24.0), ("divergence_one_field", divergence, 8.0))
    ms = {k: [] for k, _, _ in kernels}
    for rep in range(a.reps + 1):
        for k, fn, _ in kernels:
            t = timed(fn, a.calls)
            if rep:
                ms[k].append(t)
    for k, _, per in kernels:
        res[k] = dict(summary(ms[k]), bytes=per * cells)
        for q in ("median", "min", "max"):
            res[k]["tb_per_s_at_" + q] = round(per * cells / (res[k][q] * 1e-3) / 1e12, 3)
        print(json.dumps({k: res[k]}), flush=True)
    for k in ("column_water", "surface_rain"):
        res[k]["share_of_the_yardsticks_rate"] = round(res[k]["tb_per_s_at_median"] / res["divergence_one_field"]["tb_per_s_at_median"], 3)

    steps = {"step_off": [], "step_on": []}
    for rep in range(a.reps + 1):
        for k, option in (("step_off", None), ("step_on", {})):
            reset()
            micro.surface_rain = option
            t = timed(lambda: micro.time_step(c, DT), 1)
            if rep:
                steps[k].append(t)
    for k in steps:
        res[k] = summary(steps[k])
    res["step_on_minus_off_ms"] = round(res["step_on"]["median"] - res["step_off"]["median"], 4)
    res["step_on_over_off"] = round(res["step_on"]["median"] / res["step_off"]["median"], 4)
    print(json.dumps({k: res[k] for k in ("step_off", "step_on", "step_on_minus_off_ms", "step_on_over_off")}), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "surface_rain_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
