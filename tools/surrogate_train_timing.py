"""Milliseconds per epoch of the surrogate trainer at the notebook's size (9,118,906 samples -> 5,836,099 training samples, batch 1024), against
a torch-eager baseline of the same model and optimizer on the same GPU.  Run under a time limit on the MI355X:

    timeout -k 10 900 python tools/surrogate_train_timing.py --tag <tag> [--reps 3] [--n 9118906] [--models 1,8,64]

An epoch is what train_surrogate runs per epoch: the training launch, the copy of weights and sums (the host synchronisation) and the
validation pass (mw_ponni_forward + the error sums), closed here by a device synchronise.  The baseline: Linear(5,10) -> LeakyReLU(0.1) ->
Linear(10,4) in fp32, mse_loss, torch.optim.NAdam(eps=1e-7, momentum_decay=4e-3, foreach=True), a torch.randperm shuffle per epoch, data
resident on the device, the same validation set evaluated at the end of the epoch.  Warm-up epoch excluded; --reps timed epochs each;
median, min and max reported.  The data are synthetic Kessler-like samples generated on the device from a fixed seed.
Writes profiles/surrogate_train_<tag>.json.
--weighted: times the WEIGHTED epoch (mw_surrogate_train_epoch_w and the weighted validation sums; sample weights log-uniform in
[2^-4, 2^4] from a fixed seed) beside the unweighted one in the same run, on the same data, for K in 1, 8 (or --models), without the
torch baseline:    ... surrogate_train_timing.py --weighted --tag weighted_mi355x
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n, device, seed=0):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    lo = torch.tensor([200.0, 0.1, 0.0, 0.0, 0.0], device=device)
    hi = torch.tensor([300.0, 1.2, 0.02, 0.004, 0.015], device=device)
    x = lo + (hi - lo) * torch.rand((n, 5), generator=g, device=device)
    conv = 0.3 * x[:, 3] * (1.0 + torch.tanh((x[:, 0] - 250.0) / 20.0))
    y = torch.stack([x[:, 0] + 400.0 * conv, x[:, 2] + 0.2 * conv * x[:, 1], x[:, 3] - conv, x[:, 4] + 0.8 * conv], dim=1)
    return x.float().contiguous(), y.float().contiguous()


def summary(ms):
    return {"ms": [round(v, 3) for v in ms], "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "spread_pct": round(100.0 * (max(ms) - min(ms)) / statistics.median(ms), 2)}


def time_hip(raw_in, raw_out, scl_in, scl_out, n_split, K, reps, batch, sample_weights=None):
    import torch
    from miniweatherml_amd.surrogate_train import Trainer
    tr = Trainer(raw_in, raw_out, scl_in, scl_out, n_split, seed=0, models=K, batch_size=batch, epochs=1 + reps, sample_weights=sample_weights)
    tr.epoch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        tr.epoch()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    w, ts, vs = tr.finish()
    val_loss = float(vs[0].reshape(4, 6)[:, 0].sum() / (4 * n_split[1]))
    out = summary(ms)
    out.update({"models": K, "steps_per_epoch": tr.steps, "final_val_loss_model0": val_loss})
    del tr
    torch.cuda.empty_cache()
    return out


def time_torch(train, val, reps, batch):
    import torch
    tx, ty = train[0].t().contiguous(), train[1].t().contiguous()
    vx, vy = val[0].t().contiguous(), val[1].t().contiguous()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 10), torch.nn.LeakyReLU(0.1), torch.nn.Linear(10, 4)).to(tx.device)
    for lin in (model[0], model[2]):
        torch.nn.init.uniform_(lin.weight, -0.05, 0.05)
        torch.nn.init.zeros_(lin.bias)
    opt = torch.optim.NAdam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-7, momentum_decay=4e-3, foreach=True)
    n = tx.shape[0]

    def epoch():
        perm = torch.randperm(n, device=tx.device)
        tot = torch.zeros((), device=tx.device)
        for s in range(0, n, batch):
            idx = perm[s:s + batch]
            loss = torch.nn.functional.mse_loss(model(tx[idx]), ty[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            tot += loss.detach() * idx.numel()
        with torch.no_grad():
            vl = torch.nn.functional.mse_loss(model(vx), vy)
        return float(tot / n), float(vl)

    epoch()
    torch.cuda.synchronize()
    ms, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = epoch()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    out = summary(ms)
    out.update({"steps_per_epoch": (n + batch - 1) // batch, "final_loss": last[0], "final_val_loss": last[1]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--n", type=int, default=9118906)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--models", default=None, help="comma list of K (default 1,8,64; with --weighted 1,8)")
    ap.add_argument("--weighted", action="store_true", help="time the weighted epoch beside the unweighted one (no torch baseline)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from miniweatherml_amd.surrogate_train import Trainer, split_sizes
    if not torch.cuda.is_available():
        sys.exit("surrogate_train_timing: no GPU (a CPU run gives no timing)")
    dev = torch.device("cuda:0")
    raw_in, raw_out = synthetic(a.n, dev)
    scl_in = torch.stack([raw_in.min(0).values, raw_in.max(0).values], 1).double().cpu().numpy()
    scl_out = torch.stack([raw_out.min(0).values, raw_out.max(0).values], 1).double().cpu().numpy()
    n_split = split_sizes(a.n)
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "n_samples": a.n, "n_train": n_split[0],
           "n_val": n_split[1], "batch": a.batch, "reps": a.reps,
           "epoch": "training launch + copy of weights and sums + validation pass, closed by a device synchronise; warm-up epoch excluded",
           "hip": {}}
    weights = None
    if a.weighted:
        g = torch.Generator(device=dev).manual_seed(1)
        weights = torch.exp2(8.0 * torch.rand(a.n, generator=g, device=dev) - 4.0)
        res["weights"] = "log-uniform in [2^-4, 2^4], torch.Generator seed 1"
        res["hip_weighted"], res["weighted_over_unweighted"] = {}, {}
    for K in [int(k) for k in (a.models or ("1,8" if a.weighted else "1,8,64")).split(",")]:
        r = time_hip(raw_in, raw_out, scl_in, scl_out, n_split, K, a.reps, a.batch)
        res["hip"]["K%d" % K] = r
        print("HIP trainer K=%-3d  %s" % (K, json.dumps(r)), flush=True)
        if a.weighted:
            rw = time_hip(raw_in, raw_out, scl_in, scl_out, n_split, K, a.reps, a.batch, sample_weights=weights)
            res["hip_weighted"]["K%d" % K] = rw
            res["weighted_over_unweighted"]["K%d" % K] = round(rw["median_ms"] / r["median_ms"], 4)
            print("    weighted K=%-3d  %s" % (K, json.dumps(rw)), flush=True)
    if not a.no_torch and not a.weighted:
        tr = Trainer(raw_in, raw_out, scl_in, scl_out, n_split, seed=0, models=1, batch_size=a.batch, epochs=1)
        r = time_torch(tr.sets["train"], tr.sets["val"], a.reps, a.batch)
        del tr
        res["torch_eager"] = r
        print("torch eager        %s" % json.dumps(r), flush=True)
        if "K1" in res["hip"]:
            res["speedup_k1_vs_torch_eager"] = round(r["median_ms"] / res["hip"]["K1"]["median_ms"], 2)
    if "K1" in res["hip"] and "K8" in res["hip"]:
        res["k8_over_k1"] = round(res["hip"]["K8"]["median_ms"] / res["hip"]["K1"]["median_ms"], 3)
    out = a.out or os.path.join(ROOT, "profiles", "surrogate_train_%s.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
