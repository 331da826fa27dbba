"""Milliseconds per epoch of the dense-stack trainer (csrc/mw_train_stack.hip), beside the two things it can be compared
with in the same run: torch eager training the same network with the same optimizer on the same GPU, and -- for 5 -> 10 -> 4, which both
trainers can fit -- the fixed model's trainer mw_surrogate_train_epoch_v2.  Run under a time limit on the MI355X:

    timeout -k 10 900 python tools/stack_train_timing.py --tag <tag> [--reps 3] [--n 1000000]

Shapes 5 -> 32 -> 4, 5 -> 64 -> 64 -> 4, 9 -> 32 -> 4 at K = 1 and 8 models, slope 0.1, batch 1024.  An epoch, the baseline, the warm-up
epoch, the repetitions and the summary (median, min, max) are tools/surrogate_train_timing.py's; the stencil's four extra inputs are the
cell's temperature and water fields times 0.97.  Writes profiles/stack_train_<tag>.json.  No threshold: the parent cannot train a stack.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from surrogate_train_timing import summary, synthetic  # noqa: E402

SHAPES = ((5, (32,)), (5, (64, 64)), (9, (32,)))


def time_hip(data, n_split, K, reps, batch, stack):
    import torch
    from miniweatherml_amd.surrogate_train import Trainer
    tr = Trainer(*data, n_split, seed=0, models=K, batch_size=batch, epochs=1 + reps, stack=stack)
    tr.epoch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        tr.epoch()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    vs = tr.finish()[2]
    out = summary(ms)
    out.update({"models": K, "steps_per_epoch": tr.steps, "final_val_loss_model0": float(vs[0].reshape(4, 6)[:, 0].sum() / (4 * n_split[1]))})
    sets = tr.sets
    del tr
    torch.cuda.empty_cache()
    return out, sets


def time_torch(train, val, reps, batch, widths):
    import torch
    tx, ty, vx, vy = [t.t().contiguous() for t in (*train, *val)]
    torch.manual_seed(0)
    mods = []
    for a, b in zip(widths[:-2], widths[1:-1]):
        mods += [torch.nn.Linear(a, b), torch.nn.LeakyReLU(0.1)]
    model = torch.nn.Sequential(*mods, torch.nn.Linear(widths[-2], 4)).to(tx.device)
    for m in model:
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            torch.nn.init.zeros_(m.bias)
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
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from miniweatherml_amd.surrogate_train import split_sizes
    if not torch.cuda.is_available():
        sys.exit("stack_train_timing: no GPU (a CPU run gives no timing)")
    dev = torch.device("cuda:0")
    x5, y = synthetic(a.n, dev)
    x9 = torch.cat([x5, 0.97 * x5[:, (0, 2, 3, 4)]], dim=1).contiguous()
    n_split = split_sizes(a.n)
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "n_samples": a.n, "n_train": n_split[0], "n_val": n_split[1],
           "batch": a.batch, "reps": a.reps,
           "epoch": "training launch + copy of weights and sums + validation pass, closed by a device synchronise; warm-up epoch excluded", "shapes": {}}

    def data_of(x):
        scl = lambda t: torch.stack([t.min(0).values, t.max(0).values], 1).double().cpu().numpy()      # noqa: E731
        return x, y, scl(x), scl(y)

    for n_in, hidden in SHAPES + ((5, (10,)),):
        name = "-".join(str(w) for w in (n_in,) + hidden + (4,))
        data, rec = data_of(x5 if n_in == 5 else x9), {}
        for K in (1, 8):
            rec["stack_K%d" % K], sets = time_hip(data, n_split, K, a.reps, a.batch, list(hidden))
            print("%-12s stack trainer K=%d  %s" % (name, K, json.dumps(rec["stack_K%d" % K])), flush=True)
            if hidden == (10,):                                             # the fixed model's trainer on the same data
                rec["fixed_K%d" % K], _ = time_hip(data, n_split, K, a.reps, a.batch, None)
                print("%-12s fixed trainer K=%d  %s" % (name, K, json.dumps(rec["fixed_K%d" % K])), flush=True)
        if hidden != (10,):
            rec["torch_eager"] = time_torch(sets["train"], sets["val"], a.reps, a.batch, [n_in] + list(hidden) + [4])
            print("%-12s torch eager        %s" % (name, json.dumps(rec["torch_eager"])), flush=True)
            rec["speedup_k1_vs_torch_eager"] = round(rec["torch_eager"]["median_ms"] / rec["stack_K1"]["median_ms"], 2)
        res["shapes"][name] = rec
    out = a.out or os.path.join(ROOT, "profiles", "stack_train_%s.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
