"""Cost of the Kessler teacher on the rollout's model members, on a 400 x 400 x 100 state of K + 2 members
(Kessler, K models, persistence), K = 2 and K = 10:

  fused    : ms per mw_kessler_members_teacher call on the K model members (three launches and a 512-byte memset over all members'
             columns at once, the four results out of place)
  composed : the same labels from what existed before: per member mw_member_extract of the five fields to contiguous arrays and
             mw_kessler_time_step on them (in place there; nothing is copied back)

Median and min-max of --reps repetitions after one warm-up of each; every repetition is timed with device events around --calls
back-to-back calls.  Both forms start from the same state and must leave the same bits for every model member: checked once before
anything is timed.  Bytes by count: the fused form moves 72 * nens bytes per cell and call (five fields read and four written over whole
cache lines that hold all members), the composed one K * (40 * nens + 112): the extraction fetches whole lines (40 * nens), writes the
member's five arrays (40), and Kessler reads five and writes four (72).

    timeout -k 10 900 python tools/surrogate_harvest_timing.py --tag mi355x

Writes profiles/surrogate_harvest_<tag>.json (or --out).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY, NZ = 400, 400, 100
IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
HBM_MEASURED_TB_S = 6.29                     # MI355X, float4 copy


def summary(v):
    return {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def make_coupler(nens):
    import torch
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(NZ, NY, NX, nens)
    c.set_grid(1.0e5, 1.0e5, 2.0e4)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry", "temp"):
        dm.register_and_allocate(name, name, (NZ, NY, NX, nens), ["z", "y", "x", "nens"])
    modules.Microphysics_Kessler().init(c)
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    for i, name in enumerate(IN5):
        dm.get(name).copy_(si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, nens), generator=g, device="cuda:0", dtype=torch.float64))
    return c


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--models", default="2,10")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("surrogate_harvest_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd.modules import _field_ptr_array, _ptr, _stream_ptr
    L = capi.lib()
    ncells, ncol = NX * NY * NZ, NX * NY
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cells_per_member": ncells, "reps": a.reps,
           "calls_per_repetition": a.calls, "hbm_measured_TB_per_s": HBM_MEASURED_TB_S,
           "composed": "per model member: mw_member_extract of five fields + mw_kessler_time_step on the contiguous arrays, nothing copied back"}
    dt = 0.5
    for k in [int(x) for x in a.models.split(",")]:
        nens = k + 2
        members = list(range(1, k + 1))
        c = make_coupler(nens)
        dm = c.get_data_manager_readonly()
        f5 = [dm.get(n, True) for n in IN5]
        outs = [torch.empty_like(f5[0]) for _ in range(4)]
        flat = [torch.empty(ncells, dtype=torch.float64, device="cuda:0") for _ in range(5)]      # temp, density_dry, vapor, cloud, rain
        precl = torch.empty(ncol, dtype=torch.float64, device="cuda:0")
        ws = torch.empty((L.mw_kessler_workspace_bytes(NZ, ncol) + 7) // 8, dtype=torch.float64, device="cuda:0")
        st = _stream_ptr(c.device)

        def fused():
            modules.kessler_members_teacher(c, members, dt, 64, outs)

        def composed_member(m):
            capi.check(L.mw_member_extract(ncells, nens, m, 5, _field_ptr_array(f5), _field_ptr_array(flat), st))
            capi.check(L.mw_kessler_time_step(NZ, ncol, c.get_dz(), dt, _ptr(flat[2]), _ptr(flat[3]), _ptr(flat[4]), _ptr(flat[1]), _ptr(flat[0]),
                                              _ptr(precl), _ptr(ws), None, st))

        def composed():
            for m in members:
                composed_member(m)

        # the two forms leave the same bits (and warm both up)
        capi.check(L.mw_kessler_set_strict(0))
        _, rs = modules.kessler_members_teacher(c, members, dt, 64, outs, return_rainsplit=True)
        same = True
        for m in members:
            composed_member(m)
            for o, ref in zip(outs, (flat[0], flat[2], flat[3], flat[4])):
                same = same and torch.equal(o.view(-1, nens)[:, m].contiguous().view(torch.int64), ref.view(torch.int64))
        t_f, t_c = [], []
        for _ in range(a.reps):
            t_f.append(timed(fused, a.calls))
            t_c.append(timed(composed, a.calls))
        fused_bytes = 72.0 * nens * ncells
        composed_bytes = k * (40.0 * nens + 112.0) * ncells
        r = {"nens": nens, "model_members": k, "rainsplit_per_member": rs, "teacher_leaves_the_composed_bits": bool(same),
             "teacher_call": {"fused": summary(t_f), "composed": summary(t_c)},
             "bytes_per_cell_and_call": {"fused": 72 * nens, "composed": k * (40 * nens + 112)},
             "fused_GB_by_count": round(fused_bytes / 1e9, 3), "composed_GB_by_count": round(composed_bytes / 1e9, 3)}
        fm, cm = r["teacher_call"]["fused"], r["teacher_call"]["composed"]
        r["teacher_call"]["fused_over_composed"] = round(fm["median"] / cm["median"], 4)
        r["teacher_call"]["fused_faster_beyond_the_spreads"] = bool(cm["median"] - fm["median"] > (fm["max"] - fm["min"]) + (cm["max"] - cm["min"]))
        r["fused_TB_per_s_by_count"] = round(fused_bytes / (fm["median"] * 1e-3) / 1e12, 3)
        r["fused_share_of_measured_hbm_rate"] = round(r["fused_TB_per_s_by_count"] / HBM_MEASURED_TB_S, 4)
        res["K%d" % k] = r
        print("K=%-3d %s" % (k, json.dumps(r)), flush=True)
        del c, f5, outs, flat, ws
        torch.cuda.empty_cache()
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_harvest_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
