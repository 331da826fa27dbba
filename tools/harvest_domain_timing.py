"""Cost of the harvest outside the training box on a 400 x 400 x 100 state of eight members (Kessler, six
models, persistence), with surrogate_domain_timing.py's protocol for the kernels: median and min-max of --reps repetitions after one
warm-up of each, every repetition timed with device events around --calls back-to-back calls.

  plain_mask      : ms per mw_member_sample_mask call, the six model members listed (the parent's sampler), same run
  count_only      : ms per mw_member_sample_mask_domain call with mask = NULL (the harvester's first call)
  mask_domain     : ms per mw_member_sample_mask_domain call with the mask (its second call)
  copy8           : ms per plain device copy of eight fields of the state: the same-run copy rate
  harvest_plain   : ms per whole RolloutHarvester.harvest() without `outside` -- teacher, mask, nonzero, gather, the copies to the host
                    and the file appends; wall clock around a synchronised call, since the call reads back
  harvest_outside : the same with outside = {share 0.5, margin 0}

The state is a developed one in the sense of bench.py's stress state: temperature, dry density and vapour drawn over the shipped scaling
ranges, every member different, cloud and rain in blobs with sharp rims (so that the sampler meets active and inactive cells), and the
teacher values are Kessler's on it.  Each listed member's box is the shipped scaling rows with temp's upper bound at the 0.9 quantile of
the member's own temperatures: a tenth of its cells is outside.  Every second listed member has `above` set.

Bytes.  Both mask kernels issue the same thirteen 8-byte loads per listed element (five inputs, four of the level above, four teacher
values): 104 B.  The four `up` loads are the next level's own loads, 160,000 x 8 elements further on; if they are found in L2 the HBM
traffic is 72 B per listed element.  The members are interleaved, so the lines of all eight members are touched: 8/6 of that.  The mask
call writes one byte per element of all members.  The new kernel loads nothing the plain one does not: the ratio of bytes is 1.

    timeout -k 10 900 python tools/harvest_domain_timing.py --tag mi355x [--science DIR]

--science DIR: the small table of section 13.11 -- section 13.9's supercell (48 x 48 x 32, dx 1500 m), its tendency model trained on
generate_micro_data's samples, then rollout_surrogates twice for --science-steps steps: with `harvest:` alone and with `outside: true`.
Per run: eligible and taken per class (the plain run's classes are recomputed afterwards from its sample files against the same box,
on the fp32 records) and the share of the harvested samples that lie outside the box.  Writes profiles/harvest_domain_<tag>.json.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from surrogate_committee_timing import models, summary, timed  # noqa: E402
from tendency_timing import YAML  # noqa: E402

NX, NY, NZ, NENS = 400, 400, 100, 8
IN5 = ("temp", "density_dry", "water_vapor", "cloud_liquid", "precip_liquid")
DT = 0.5


def make_coupler():
    import torch
    from miniweatherml_amd import modules
    from miniweatherml_amd.coupler import Coupler
    c = Coupler("cuda:0")
    c.distribute_mpi_and_allocate_coupled_state(NZ, NY, NX, NENS)
    c.set_grid(500.0 * NX, 500.0 * NY, 2.0e4)
    dm = c.get_data_manager_readwrite()
    for name in ("density_dry", "temp"):
        dm.register_and_allocate(name, name, (NZ, NY, NX, NENS), ["z", "y", "x", "nens"])
    modules.Microphysics_Kessler().init(c)
    si = modules.load_surrogate_weights()[4]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    for i, name in enumerate(IN5[:3]):
        dm.get(name).copy_(si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY, NX, NENS), generator=g, device="cuda:0", dtype=torch.float64))
    rho_d = dm.get("density_dry")
    k = torch.arange(NZ, device="cuda:0", dtype=torch.float64).view(NZ, 1, 1, 1)
    j = torch.arange(NY, device="cuda:0", dtype=torch.float64).view(1, NY, 1, 1)
    i = torch.arange(NX, device="cuda:0", dtype=torch.float64).view(1, 1, NX, 1)
    e = torch.arange(NENS, device="cuda:0", dtype=torch.float64).view(1, 1, 1, NENS)
    blob = ((torch.sin(i * 0.11 + e) * torch.cos(j * 0.07)) > 0.3).to(torch.float64)                   # bench.py's blobs, shifted per member
    dm.get("cloud_liquid").copy_(2.0e-3 * blob * ((k > 0.15 * NZ) & (k < 0.45 * NZ)) * (0.5 + 0.5 * torch.sin(0.3 * k + 0.05 * i) ** 2) * rho_d)
    dm.get("precip_liquid").copy_(4.0e-4 * blob * (k < 0.3 * NZ) * (0.5 + 0.5 * torch.cos(0.2 * k + 0.03 * j) ** 2) * rho_d)
    return c


def wall(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1.0e3 * (time.perf_counter() - t0) / calls


def timings(a, res):
    import numpy as np
    import torch
    from miniweatherml_amd import capi, modules
    from miniweatherml_amd.modules import _field_ptr_array, _stream_ptr
    L = capi.lib()
    ncol, ncells = NX * NY, NX * NY * NZ
    members = list(range(1, NENS - 1))
    nm = len(members)
    c = make_coupler()
    dm = c.get_data_manager_readonly()
    f5 = [dm.get(n, True) for n in IN5]
    teacher, rs = modules.kessler_members_teacher(c, members, DT, 64, return_rainsplit=True)
    if min(rs) < 1:
        sys.exit("harvest_domain_timing: the teacher skipped a member (%r)" % (rs,))
    si = modules.load_surrogate_weights()[4]
    boxes = np.tile(np.asarray(si, dtype=np.float64), (nm, 1, 1))
    for j, m in enumerate(members):
        boxes[j, 0, 1] = float(torch.quantile(f5[0][0, :, :, m].flatten()[:1000000], 0.9))
    above = [j % 2 == 1 for j in range(nm)]
    nelem = ncells * NENS
    mask = torch.empty(nelem, dtype=torch.uint8, device="cuda:0")
    counts = torch.empty((nm, 6), dtype=torch.int64, device="cuda:0")
    key0 = 7 * nelem
    share, sps = 0.5, 50.0

    def measure(fn):
        timed(fn, a.calls)
        return summary([timed(fn, a.calls) for _ in range(a.reps)])

    modules.member_sample_mask_domain(NZ, f5, teacher, members, boxes, above, key0, np.zeros((nm, 3)), None, counts)
    first = counts.cpu().numpy()
    thr = np.array([modules.harvest_thresholds(sps, 0.5, 0.4, ncells, share, int(q)) for q in first[:, 0]])
    cm = (C.c_int * nm)(*members)
    rows = {}
    rows["plain_mask"] = measure(lambda: capi.check(L.mw_member_sample_mask(NZ, ncol, NENS, nm, cm, _field_ptr_array(f5), _field_ptr_array(teacher),
                                                                             key0, float(thr[0, 1]), float(thr[0, 2]), C.c_void_p(mask.data_ptr()),
                                                                             _stream_ptr(c.device))))
    rows["count_only"] = measure(lambda: modules.member_sample_mask_domain(NZ, f5, teacher, members, boxes, above, key0, thr, None, counts))
    rows["mask_domain"] = measure(lambda: modules.member_sample_mask_domain(NZ, f5, teacher, members, boxes, above, key0, thr, mask, counts))
    last = counts.cpu().numpy()
    if not np.array_equal(last[:, :3], first[:, :3]) or int(mask.sum()) != int(last[:, 3:].sum()):
        sys.exit("harvest_domain_timing: the mask call's counts contradict the count-only call's or the mask")
    dst = [torch.empty_like(f5[0]) for _ in range(8)]
    src = f5 + teacher[:3]

    def copy8():
        for s, d in zip(src, dst):
            d.copy_(s)
    rows["copy8"] = measure(copy8)
    del dst
    torch.cuda.empty_cache()
    rate = lambda nbytes, row: nbytes / (row["median"] * 1e-3) / 1e12                                  # noqa: E731   TB/s
    listed = float(nm) * ncells
    res["counts_per_member"] = {"eligible_outside_active_inactive": first[:, :3].tolist(), "taken": last[:, 3:].tolist(), "thresholds": thr.tolist()}
    res["bytes_per_listed_element"] = {"issued": 104, "from_hbm_if_the_up_loads_hit_l2": 72, "touched_lines_factor": round(NENS / nm, 4),
                                       "mask_bytes_per_element_of_all_members": 1}
    res["same_run_copy_rate_TB_s"] = round(rate(2 * 64.0 * ncells * NENS, rows["copy8"]), 4)
    res["rate_TB_s"] = {k: {"issued_104B": round(rate(104.0 * listed, rows[k]), 4), "hbm_72B_listed": round(rate(72.0 * listed, rows[k]), 4),
                            "hbm_72B_touched_lines": round(rate(72.0 * ncells * NENS + (0 if k == "count_only" else nelem), rows[k]), 4)}
                        for k in ("plain_mask", "count_only", "mask_domain")}
    res["ratio_of_bytes_mask_domain_over_plain_mask"] = 1.0
    res["mask_domain_over_plain_mask_ms"] = round(rows["mask_domain"]["median"] / rows["plain_mask"]["median"], 4)
    res["count_only_over_plain_mask_ms"] = round(rows["count_only"]["median"] / rows["plain_mask"]["median"], 4)
    # ---- the whole harvest() ---------------------------------------------------------------------------------------------------------
    names = ["m%d" % m for m in members]
    for key, kw in (("harvest_plain", {}), ("harvest_outside", dict(outside={"share": share, "margin": 0.0, "fields": list(IN5)}, boxes=boxes,
                                                                        above=above))):
        with tempfile.TemporaryDirectory() as d:
            h = modules.RolloutHarvester()
            h.init(c, names, members, d, samples_per_step=sps if not kw else sps / (1 - share), seed=3, **kw)
            wall(lambda: h.harvest(c, DT, 0.0), 1)
            rows[key] = summary([wall(lambda: h.harvest(c, DT, 0.0), a.calls) for _ in range(a.reps)])
            rows[key]["samples_per_call"] = round(sum(h.samples.values()) / float(h.calls), 2)
    res["harvest_outside_minus_plain_ms"] = round(rows["harvest_outside"]["median"] - rows["harvest_plain"]["median"], 4)
    res["rows"] = rows
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    print(json.dumps({k: [v["median"], v["min"], v["max"]] for k, v in rows.items()}), flush=True)


def science(a, res):
    import numpy as np
    from miniweatherml_amd import driver, modules, surrogate_train as st
    work = os.path.abspath(a.science)
    os.makedirs(work, exist_ok=True)
    here = os.getcwd()
    os.chdir(work)
    try:
        kw = dict(n=48, nz=32, xlen=1500.0 * 48, prefix=os.path.join(work, "out"))
        path = os.path.join(work, "generate.yaml")
        open(path, "w").write(YAML.format(nens=1, extra="", **kw))
        _, _, info = driver.run("generate_micro_data", path, max_steps=a.science_steps, quiet=True)
        sample_file = os.path.join(work, "supercell_kessler_data_task_0.nc")
        r = st.train_surrogate([sample_file], os.path.join(work, "tendency"), epochs=a.science_epochs, batch_size=256, seed=0, models=2, form="tendency")
        p = r["files_written"]
        print("harvest_domain_timing: science: %d samples, trained" % int(info["samples"]), flush=True)
        extra = 'surrogate_models:\n  - {name: tendency, keras_weights_txt: "%s", nn_input_scaling: "%s", nn_output_scaling: "%s"}\n' % tuple(p)
        extra += "eval_interval: 100\n"
        box = modules.domain_box([modules.load_surrogate_model(*p)])
        sci = {"grid": [48, 48, 32], "dx": 1500.0, "steps": a.science_steps, "samples_trained_on": int(info["samples"]), "epochs": a.science_epochs,
               "harvest": {"interval": 100, "samples_per_step": 200, "seed": 1}, "box": modules.box_json(box), "runs": {}}
        for key, option in (("plain", ""), ("outside", ", outside: true")):
            d = os.path.join(work, key)
            os.makedirs(d, exist_ok=True)
            os.chdir(d)
            path = os.path.join(d, "rollout.yaml")
            open(path, "w").write(YAML.format(nens=3, extra=extra + "harvest: {interval: 100, samples_per_step: 200, seed: 1%s}\n" % option, **kw))
            driver.run("rollout_surrogates", path, max_steps=a.science_steps, quiet=True)
            doc = json.load(open(os.path.join(d, "surrogate_rollout.json")))
            hv = doc["harvest"]
            x = st.read_samples([hv["files"]["tendency"]])[0].astype(np.float64)                       # the fp32 records against the fp64 box
            out = ((x < box[:, 0]) | (x > box[:, 1])).any(axis=1)
            run = {"calls": hv["calls"], "skipped": hv["skipped"]["tendency"], "samples": int(x.shape[0]), "samples_outside_the_box": int(out.sum()),
                   "share_of_samples_outside": float(out.mean()) if x.shape[0] else None, "diverged_at": doc["diverged_at"]["tendency"]}
            if "taken" in hv:
                run["taken"], run["eligible"] = hv["taken"]["tendency"], hv["eligible"]["tendency"]
            sci["runs"][key] = run
            print(json.dumps({key: run}), flush=True)
        res["science"] = sci
    finally:
        os.chdir(here)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--science", default=None, metavar="DIR")
    ap.add_argument("--science-steps", type=int, default=4000)
    ap.add_argument("--science-epochs", type=int, default=20)
    ap.add_argument("--science-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("harvest_domain_timing: no GPU (a CPU run gives no timing)")
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cells_per_member": NX * NY * NZ, "members": NENS,
           "listed_members": NENS - 2, "reps": a.reps, "calls_per_repetition": a.calls}
    out = a.out or os.path.join(ROOT, "profiles", "harvest_domain_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def write():
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    if not a.science_only:
        timings(a, res)
        write()
    if a.science:
        science(a, res)
        write()
    print("wrote", out)


if __name__ == "__main__":
    main()
