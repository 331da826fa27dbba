"""What a dense surrogate stack costs on the fused stack kernel, on 400 x 400 x 100 cells:

  5 -> 10 -> 4          : mw_mlp_stack_forward against mw_mlp_forward with the same weights, interleaved in one run
  5 -> 32 -> 4          : the stack kernel against torch fp32 eager on the device for the same stack (scale in fp64, cast, Linear /
  5 -> 64 -> 64 -> 4      leaky_relu chain in fp32, un-scale and clip in fp64 -- what a user without the kernel would write), interleaved
  9 -> 32 -> 4          : the stack kernel alone (features 5..8 are plain loads of the level above)

Every timing: one warm-up repetition, then --reps repetitions of --calls back-to-back calls between two device events, the variants
alternating inside a repetition; medians and [min, max].  Beside each stack: the MFMAs per 16-cell tile its shape implies, the fp32
matrix rate that makes of the median (2048 flop per MFMA, padding included) and the HBM rate at 72 bytes per cell.

    timeout -k 10 600 python tools/mlp_stack_timing.py --tag mi355x

Writes profiles/mlp_stack_<tag>.json (or --out) and prints the table of section 13.18.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tendency_timing import interleaved  # noqa: E402

NX, NY, NZ = 400, 400, 100
CASES = [(5, [10]), (5, [32]), (5, [64, 64]), (9, [32])]


def random_stack(n_in, widths, si, so, seed):
    import numpy as np
    from miniweatherml_amd import mlp
    rng = np.random.default_rng(seed)
    w = [n_in] + widths + [4]
    layers = [((rng.uniform(-1, 1, (a, b)) * np.sqrt(6.0 / (a + b))).astype(np.float32), np.zeros(b, np.float32)) for a, b in zip(w[:-1], w[1:])]
    si = si if n_in == 5 else np.ascontiguousarray(np.concatenate([si, si[[0, 2, 3, 4]]]))
    return mlp.SurrogateStack(layers, [0.1] * len(widths), si, so, "state")


def mfmas_per_tile(widths):
    return sum(-(-a // 4) * -(-b // 16) for a, b in zip(widths[:-1], widths[1:]))


def torch_eager(stack, ins):
    """The same stack in eager torch on the device: fp64 scaling, fp32 layers, fp64 un-scaling and clip."""
    import torch
    dev = ins[0].device
    Ws = [(torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)) for W, b in stack.layers]
    lo, rng = torch.from_numpy(stack.scl_in[:, 0]).to(dev), torch.from_numpy(stack.scl_in[:, 1] - stack.scl_in[:, 0]).to(dev)
    olo, orng = torch.from_numpy(stack.scl_out[:, 0]).to(dev), torch.from_numpy(stack.scl_out[:, 1] - stack.scl_out[:, 0]).to(dev)

    def fn():
        x = ((torch.stack(ins, 1) - lo) / rng).float()
        for l, (W, b) in enumerate(Ws):
            x = torch.addmm(b, x, W)
            if l < len(Ws) - 1:
                x = torch.nn.functional.leaky_relu(x, float(stack.slopes[l]))
        y = x.double() * orng + olo
        y[:, 1:].clamp_(min=0.0)
        return y
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mlp_stack_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import mlp, modules
    n = NX * NY * NZ
    W1, b1, W2, b2, si, so = modules.load_surrogate_weights()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    ins = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand(n, generator=g, device="cuda:0", dtype=torch.float64) for i in range(5)]
    outs = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "reps": a.reps,
           "calls_per_repetition": a.calls, "cases": {}}
    for n_in, widths in CASES:
        key = " -> ".join(str(w) for w in [n_in] + widths + [4])
        stack = random_stack(n_in, widths, si, so, 0)
        if (n_in, widths) == (5, [10]):
            stack = stack._replace(layers=[(W1, b1), (W2, b2)])
        h = mlp.MlpStack(stack, "cuda:0")
        v = [("stack", lambda: h.forward(NZ, *ins, outs=outs))]
        if (n_in, widths) == (5, [10]):
            v.append(("mw_mlp_forward", lambda: modules.mlp_forward(*ins, W1, b1, W2, b2, si, so, outs=outs)))
        elif n_in == 5:
            eager = torch_eager(stack, ins)
            want = eager()
            h.forward(NZ, *ins, outs=outs)
            worst = max(float((outs[k] - want[:, k]).abs().max() / (so[k, 1] - so[k, 0])) for k in range(4))
            del want
            v.append(("torch_fp32_eager", eager))
        r = interleaved(v, a.reps, a.calls)
        m = mfmas_per_tile([n_in] + widths + [4])
        r["mfma_per_tile"] = m
        r["stack_matrix_tflops_padding_included"] = round(m * 2048.0 * (n / 16.0) / (r["stack"]["median"] * 1e-3) / 1e12, 2)
        r["stack_tb_per_s_at_72_bytes_per_cell"] = round(72.0 * n / (r["stack"]["median"] * 1e-3) / 1e12, 3)
        if "torch_fp32_eager" in r:
            r["max_scaled_difference_to_eager"] = worst
        res["cases"][key] = r
        print(json.dumps({key: r}), flush=True)
        h.close()
    out = a.out or os.path.join(ROOT, "profiles", "mlp_stack_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("%-20s %6s %28s %28s %8s %8s" % ("ms per call", "MFMA", "stack", "other", "TFLOP/s", "TB/s"))
    for key, r in res["cases"].items():
        other = [k for k in ("mw_mlp_forward", "torch_fp32_eager") if k in r]
        cell = lambda k: "%.4f [%.4f, %.4f]" % (r[k]["median"], r[k]["min"], r[k]["max"])     # noqa: E731
        print("%-20s %6d %28s %28s %8.2f %8.3f" % (key, r["mfma_per_tile"], cell("stack"), (other[0] + " " + cell(other[0])) if other else "-",
                                                   r["stack_matrix_tflops_padding_included"], r["stack_tb_per_s_at_72_bytes_per_cell"]))
    print("wrote", out)


if __name__ == "__main__":
    main()
