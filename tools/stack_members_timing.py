"""What stepping dense stacks as ensemble members costs, on 400 x 400 x 100 cells with nens = 8, for the stacks
5 -> 32 -> 4, 9 -> 32 -> 4 and 5 -> 64 -> 64 -> 4 on one, four and six members:

  in_place   : one MlpStackGroup.members_apply call for all the members (mw_stack_group_members_apply)
  composed   : what there was before it, per member mw_member_extract of five fields, mw_mlp_stack_forward to four scratch fields and
               mw_member_insert of four, on the same state in the same run
  contiguous : mw_mlp_stack_forward alone on the extracted member's contiguous fields, once per member (no strided access at all)

Every timing: one warm-up repetition, then --reps repetitions of --calls back-to-back calls between two device events, the variants
alternating inside a repetition; medians and [min, max].  Bytes per cell and member that the step needs: 5 fields read, 4 written, 72 B;
the composed form moves 5 x 16 + 72 + 4 x 16 = 216 B.  TB/s is 72 B per cell and member over the median.

    timeout -k 10 900 python tools/stack_members_timing.py --tag mi355x

Writes profiles/stack_members_<tag>.json (or --out) and prints the table of section 13.20.
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

NX, NY, NZ, NENS = 400, 400, 100, 8
SHAPES = [(5, [32]), (9, [32]), (5, [64, 64])]
MEMBERS = (1, 4, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="local")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stack_members_timing: no GPU (a CPU run gives no timing)")
    from miniweatherml_amd import capi, mlp, modules
    from miniweatherml_amd._ffi import _field_ptr_array, _stream_ptr
    n = NX * NY * NZ
    _, _, _, _, si, so = modules.load_surrogate_weights()
    g = torch.Generator(device="cuda:0").manual_seed(0)
    order = (0, 1, 2, 3, 4)                                                # temp, density_dry, water_vapor, cloud_liquid, precip_liquid = the rows of si
    f5 = [si[i, 0] + (si[i, 1] - si[i, 0]) * torch.rand((NZ, NY * NX, NENS), generator=g, device="cuda:0", dtype=torch.float64) for i in order]
    ext = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(5)]
    outs = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    L, st = capi.lib(), _stream_ptr(f5[0].device)
    res = {"tag": a.tag, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "nx": NX, "ny": NY, "nz": NZ, "nens": NENS,
           "reps": a.reps, "calls_per_repetition": a.calls, "bytes_per_cell_and_member": {"in_place": 72, "composed": 216, "contiguous": 72}, "cases": {}}
    for n_in, widths in SHAPES:
        stack = random_stack(n_in, widths, si, so, 0)
        handle = mlp.MlpStack(stack, "cuda:0")
        for k in MEMBERS:
            key = "%s x %d" % (" -> ".join(str(w) for w in [n_in] + widths + [4]), k)
            members = list(range(1, 1 + k))
            group = mlp.MlpStackGroup([handle] * k, "cuda:0")

            def composed():
                for e in members:
                    capi.check(L.mw_member_extract(n, NENS, e, 5, _field_ptr_array(f5), _field_ptr_array(ext), st))
                    handle.forward(NZ, *ext, outs=outs)
                    capi.check(L.mw_member_insert(n, NENS, e, 4, _field_ptr_array(outs), _field_ptr_array([f5[0], f5[2], f5[3], f5[4]]), st))

            def contiguous():
                for e in members:
                    handle.forward(NZ, *ext, outs=outs)

            capi.check(L.mw_member_extract(n, NENS, 1, 5, _field_ptr_array(f5), _field_ptr_array(ext), st))
            r = interleaved([("in_place", lambda: group.members_apply(NZ, members, f5)), ("composed", composed), ("contiguous", contiguous)],
                            a.reps, a.calls)
            for v in ("in_place", "composed", "contiguous"):
                r[v]["tb_per_s_at_72_bytes"] = round(72.0 * n * k / (r[v]["median"] * 1e-3) / 1e12, 3)
            r["in_place_within_composed_spread"] = r["in_place"]["median"] <= r["composed"]["median"] + (r["composed"]["max"] - r["composed"]["min"])
            res["cases"][key] = r
            print(json.dumps({key: r}), flush=True)
            group.close()
        handle.close()
    out = a.out or os.path.join(ROOT, "profiles", "stack_members_%s.json" % a.tag)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    cell = lambda r: "%.3f [%.3f, %.3f] %5.2f" % (r["median"], r["min"], r["max"], r["tb_per_s_at_72_bytes"])     # noqa: E731
    print("%-26s %30s %30s %30s" % ("ms per call, TB/s", "in_place", "composed", "contiguous"))
    for key, r in res["cases"].items():
        print("%-26s %30s %30s %30s" % (key, cell(r["in_place"]), cell(r["composed"]), cell(r["contiguous"])))
    print("wrote", out)


if __name__ == "__main__":
    main()
