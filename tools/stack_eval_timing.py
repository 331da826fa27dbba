"""What scoring dense stacks against the truth fields costs, on 400 x 400 x 100 cells with half the cells
active, for the groups 5 -> 32 -> 4 x {1, 4, 8}, 9 -> 32 -> 4 x {1, 4} and 5 -> 64 -> 64 -> 4 x {1, 4}:

  fused    : one MlpStackGroup.evaluate-style call for the whole group (mw_stack_group_eval on a kept workspace, no host copy)
  composed : what there was before it, per stack mw_mlp_stack_forward into four temporaries and torch reductions for the 32 numbers
             (class masks, d, |d|, d^2, sums and maxima), with the one host copy per stack that fetches them
  forward  : mw_mlp_stack_forward alone, once per stack -- the floor: the network without any statistic

Every timing: one warm-up repetition, then --reps repetitions of --calls back-to-back calls between two device events, the variants
alternating inside a repetition; medians and [min, max].  Bytes per cell that a pass over the state needs: 5 input and 4 truth fields,
72 B; the fused call makes one pass per workgroup of mpb stacks (plus one for persistence), the other two one pass per stack.  TB/s is
72 B per cell and pass over the median.

    timeout -k 10 900 python tools/stack_eval_timing.py --tag mi355x

Writes profiles/stack_eval_<tag>.json (or --out) and prints the table of section 13.21.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mlp_stack_timing import random_stack  # noqa: E402
from tendency_timing import interleaved  # noqa: E402

NX, NY, NZ = 400, 400, 100
GROUPS = [(5, [32], 1), (5, [32], 4), (5, [32], 8), (9, [32], 1), (9, [32], 4), (5, [64, 64], 1), (5, [64, 64], 4)]
BEFORE = (0, 2, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stack_eval_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, mlp, modules
    from miniweatherml_amd._ffi import StatsAndCounts, _field_ptr_array, _ptr, _stream_ptr, fit_workspace
    n, ncol = NX * NY * NZ, NX * NY
    _, _, _, _, si, so = modules.load_surrogate_weights()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    in5 = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, ncol), generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    act = torch.rand((NZ, ncol), generator=g, device="cuda:0") < 0.5
    truth4 = [torch.where(act, in5[b] * 1.001 + 1e-6, in5[b]) for b in BEFORE]
    outs = [torch.empty_like(in5[0]) for _ in range(4)]
    L, st = capi.lib(), _stream_ptr(in5[0].device)
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "active_share": float(act.double().mean()),
           "reps": a.reps, "calls_per_repetition": a.calls, "bytes_per_cell_and_pass": 72, "cases": {}}
    for n_in, widths, k in GROUPS:
        key = "%s x %d" % (" -> ".join(str(w) for w in [n_in] + widths + [4]), k)
        handle = mlp.MlpStack(random_stack(n_in, widths, si, so, 0), "cuda:0")
        group = mlp.MlpStackGroup([handle] * k, "cuda:0")
        ws = fit_workspace(None, L.mw_stack_group_eval_workspace_bytes(group._h, NZ, ncol), "cuda:0")
        buf = StatsAndCounts((k + 1) * 32, 2, "cuda:0")

        def fused():
            capi.check(L.mw_stack_group_eval(group._h, NZ, ncol, _field_ptr_array(in5), _field_ptr_array(truth4), buf.stats_ptr, buf.counts_ptr, _ptr(ws), st))

        def composed():
            active = torch.zeros_like(act)
            for v, b in enumerate(BEFORE):
                active |= (truth4[v] - in5[b]).abs() > 1e-10
            for _ in range(k):
                handle.forward(NZ, *in5, outs=outs)
                rows = []
                for v in range(4):
                    d = outs[v] - truth4[v]
                    for mask in (~active, active):
                        dm = torch.where(mask, d, torch.zeros_like(d))
                        rows.append(torch.stack([dm.sum(), dm.abs().sum(), (dm * dm).sum(), dm.abs().max()]))
                torch.stack(rows).cpu()

        def forward():
            for _ in range(k):
                handle.forward(NZ, *in5, outs=outs)

        r = interleaved([("fused", fused), ("composed", composed), ("forward", forward)], a.reps, a.calls)
        mpb = 4 if k >= 3 else k
        passes = {"fused": -(-k // mpb) + 1, "composed": k, "forward": k}
        for v in passes:
            r[v]["passes"] = passes[v]
            r[v]["tb_per_s_at_72_bytes"] = round(72.0 * n * passes[v] / (r[v]["median"] * 1e-3) / 1e12, 3)
        r["fused_over_composed"] = round(r["fused"]["median"] / r["composed"]["median"], 4)
        r["fused_over_forward"] = round(r["fused"]["median"] / r["forward"]["median"], 4)
        res["cases"][key] = r
        print(json.dumps({key: r}), flush=True)
        group.close()
        handle.close()
    out = a.out or os.path.join(ROOT, "profiles", "stack_eval_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    cell = lambda r: "%.3f [%.3f, %.3f] %5.2f" % (r["median"], r["min"], r["max"], r["tb_per_s_at_72_bytes"])     # noqa: E731
    print("%-26s %30s %30s %30s" % ("ms per call, TB/s", "fused", "composed", "forward"))
    for key, r in res["cases"].items():
        print("%-26s %30s %30s %30s" % (key, cell(r["fused"]), cell(r["composed"]), cell(r["forward"])))
    print("wrote", out)


if __name__ == "__main__":
    main()
