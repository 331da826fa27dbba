"""Cost of rolling K candidate surrogates out as ensemble members, on a 400 x 400 x 100 state of K + 2 members
(Kessler, K models of both widths alternating, persistence), K = 2 and K = 10:

  fused    : ms per Microphysics_Rollout.time_step (member 0 out, Kessler, member 0 back, one mw_surrogate_members_apply per width) and per
             modules.member_divergence call over the eight coupler fields (two launches and the device-to-host copy of the result)
  composed : the same from what existed before.  Step: member 0's six arrays made contiguous with torch, Microphysics_Kessler's entry on
             them, copied back; per model the member's five slices made contiguous, the existing forward into four temporaries, four
             copies back.  Statistics: per field torch reductions over the (cells, members) view -- d = x - x[:, :1], sum d, sum |d|,
             sum d^2, amax |d|, sum x, amin x, amax x, and the count of non-finite elements -- and one host copy.

Median and min-max of --reps repetitions after one warm-up of each; every repetition is timed with device events around --calls
back-to-back calls (the divergence and the composed statistics, which end in a host copy, with the host clock).  The fused and the
composed step start from the same state and must leave the same bits: checked once before anything is timed.

    timeout -k 10 900 python tools/surrogate_rollout_timing.py --tag mi355x

Writes profiles/surrogate_rollout_<tag>.json (or --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY, NZ = 400, 400, 100
IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
HBM_MEASURED_TB_S = 6.29                     # MI355X, float4 copy


def summary(v):
    return {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def models(k):
    """k models, stencil and single-cell alternating, fresh draws with the shipped scaling tables."""
    import numpy as np
    from miniweatherml_amd import modules, surrogate_train as st
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    si9 = np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]]))
    out = []
    for i in range(k):
        nine = i % 2 == 0
        p = st.split_weights(st.initial_weights(i, 1, stencil=nine)[0])
        out.append((np.ascontiguousarray(p[0]), p[1].copy(), np.ascontiguousarray(p[2]), p[3].copy(), si9 if nine else si, so))
    return out


def make_coupler(nens, micro, **init):
    import torch
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(NZ, NY, NX, nens)
    c.set_grid(1.0e5, 1.0e5, 2.0e4)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry", "uvel", "vvel", "wvel", "temp"):
        dm.register_and_allocate(name, name, (NZ, NY, NX, nens), ["z", "y", "x", "nens"])
    micro.init(c, **init)
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    for i, name in enumerate(IN5):
        dm.get(name).copy_(si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, nens), generator=g, device="cuda:0", dtype=torch.float64))
    for name in ("uvel", "vvel", "wvel"):
        dm.get(name).copy_(20.0 * torch.rand((NZ, NY, NX, nens), generator=g, device="cuda:0", dtype=torch.float64) - 10.0)
    return c


def composed_step(coupler, kessler, nets, dt):
    """The rollout step from the entry points that existed before."""
    from miniweatherml_amd import modules
    dm = coupler.get_data_manager_readwrite()
    f = {n: dm.get(n) for n in IN5 + ("precl",)}
    one = kessler["coupler"].get_data_manager_readwrite()
    for n in IN5 + ("precl",):
        one.get(n).copy_(f[n][..., 0:1])
    kessler["micro"].time_step(kessler["coupler"], dt)
    for n in ("temp", "water_vapor", "cloud_liquid", "precip_liquid", "precl"):
        f[n][..., 0:1].copy_(one.get(n))
    for k, net in enumerate(nets):
        ins = [f[n][..., 1 + k].contiguous() for n in IN5]
        if net[0].shape[0] == 9:
            outs = modules.mlp_stencil_forward(NZ, *ins, *net, outs=kessler["tmp"])
        else:
            outs = modules.mlp_forward(*ins, *net, outs=kessler["tmp"])
        for n, o in zip(("temp", "water_vapor", "cloud_liquid", "precip_liquid"), outs):
            f[n][..., 1 + k].copy_(o)


def composed_divergence(coupler, names):
    import torch
    dm = coupler.get_data_manager_readonly()
    nens = coupler.get_nens()
    rows = []
    for n in names:
        x = dm.get(n, True).view(-1, nens)
        d = x - x[:, :1]
        ad = d.abs()
        rows.append(torch.stack([d.sum(0), ad.sum(0), (d * d).sum(0), ad.amax(0), x.sum(0), x.amin(0), x.amax(0),
                                 (~torch.isfinite(x)).sum(0).to(torch.float64)]))
    return torch.stack(rows).cpu().numpy()


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def host_timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


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
        sys.exit("surrogate_rollout_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import modules
    ncells = NX * NY * NZ
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cells_per_member": ncells, "reps": a.reps,
           "calls_per_repetition": a.calls, "hbm_measured_TB_per_s": HBM_MEASURED_TB_S,
           "composed": "member 0 contiguous + Microphysics_Kessler + copy back; per model five contiguous slices, the existing forward, four copies "
                       "back; statistics by torch reductions per field"}
    dt = 0.5
    for k in [int(x) for x in a.models.split(",")]:
        nens = k + 2
        nets = models(k)
        micro = modules.Microphysics_Rollout()
        c = make_coupler(nens, micro, models=nets, persistence=True)
        kes = {"micro": modules.Microphysics_Kessler()}
        kes["coupler"] = make_coupler(1, kes["micro"])
        kes["tmp"] = [torch.empty((NZ, NY, NX), dtype=torch.float64, device="cuda:0") for _ in range(4)]
        dm = c.get_data_manager_readwrite()
        start = {n: dm.get(n).clone() for n in IN5}
        # the two forms leave the same bits (and warm both up)
        micro.time_step(c, dt)
        fused_bits = [dm.get(n).clone() for n in IN5]
        for n in IN5:
            dm.get(n).copy_(start[n])
        composed_step(c, kes, nets, dt)
        same = all(torch.equal(x.view(torch.int64), dm.get(n).view(torch.int64)) for x, n in zip(fused_bits, IN5))
        got = modules.member_divergence(c, modules.ROLLOUT_FIELDS)
        ref = composed_divergence(c, modules.ROLLOUT_FIELDS)
        fin = abs(ref[:, :7]) > 0
        rel = float(abs(got[0].transpose(1, 2, 0)[:, :7][fin] - ref[:, :7][fin]).max() / abs(ref[:, :7][fin]).max())
        del fused_bits
        step_f, step_c, div_f, div_c = [], [], [], []
        for _ in range(a.reps):
            step_f.append(timed(lambda: micro.time_step(c, dt), a.calls))
            step_c.append(timed(lambda: composed_step(c, kes, nets, dt), a.calls))
            div_f.append(host_timed(lambda: modules.member_divergence(c, modules.ROLLOUT_FIELDS)))
            div_c.append(host_timed(lambda: composed_divergence(c, modules.ROLLOUT_FIELDS)))
        n5 = sum(1 for m in nets if m[0].shape[0] == 5)
        # bytes the algorithm needs: the models read five fields and write four of their member; member 0 goes out (5 + precl), through
        # Kessler (5 read, 4 written, of contiguous arrays) and back (4); the divergence reads every element of eight fields once
        apply_bytes = 72.0 * ncells * k
        member0_bytes = (5 * 16.0 + 72.0 + 4 * 16.0) * ncells
        div_bytes = 8.0 * 8 * ncells * nens
        r = {"nens": nens, "single_cell_models": n5, "stencil_models": k - n5, "step_leaves_the_composed_bits": bool(same),
             "divergence_vs_torch_max_rel_diff": rel,
             "rollout_step": {"fused": summary(step_f), "composed": summary(step_c)},
             "member_divergence_8_fields": {"fused": summary(div_f), "composed": summary(div_c)},
             "bytes_per_cell_and_model_members_apply": 72, "bytes_per_cell_and_member_divergence_8_fields": 64,
             "step_GB_needed": round((apply_bytes + member0_bytes) / 1e9, 3), "divergence_GB_needed": round(div_bytes / 1e9, 3)}
        r["rollout_step"]["fused_over_composed"] = round(r["rollout_step"]["fused"]["median"] / r["rollout_step"]["composed"]["median"], 4)
        r["member_divergence_8_fields"]["fused_over_composed"] = round(r["member_divergence_8_fields"]["fused"]["median"] /
                                                                       r["member_divergence_8_fields"]["composed"]["median"], 4)
        r["step_share_of_measured_hbm_rate"] = round((apply_bytes + member0_bytes) / (r["rollout_step"]["fused"]["median"] * 1e-3) / (HBM_MEASURED_TB_S * 1e12), 4)
        r["divergence_share_of_measured_hbm_rate"] = round(div_bytes / (r["member_divergence_8_fields"]["fused"]["median"] * 1e-3) / (HBM_MEASURED_TB_S * 1e12), 4)
        res["K%d" % k] = r
        print("K=%-3d %s" % (k, json.dumps(r)), flush=True)
        del c, kes, micro, start
        torch.cuda.empty_cache()
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_rollout_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
