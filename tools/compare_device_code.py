"""Is the gfx950 code of every kernel the same in two checkouts?  (no GPU needed; for refactors that move kernels between units)

    python tools/compare_device_code.py --base <other checkout>/miniweatherml_amd/csrc [--csrc DIR] [--jobs N] [--keep DIR] [--rename OLD=NEW ...]

Compiles every *.hip of both csrc directories to device assembly (hipcc -S --offload-device-only, the flags of build.py, with
-Rpass-analysis=kernel-resource-usage) and compares, per function of the code objects (kernels and the out-of-line device functions):
  * the instruction stream, after stripping comments, directives and the function number of block labels (.LBB<fn>_<n>);
  * the resource remark: VGPRs, AGPRs, SGPRs, spills, scratch, occupancy, LDS.
A kernel that one side defines in more than one unit is reported (without relocatable device code it would sit in the library twice).
--rename OLD=NEW (mangled names, may be repeated): the base's function OLD is compared with the new side's NEW -- a kernel that only
changed its name, say into a template instance.
Exit status 0 when everything is equal.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-ffp-contract=on", "-I/opt/rocm/include"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_unit(job):
    csrc, src, out = job
    cmd = [HIPCC] + FLAGS + ["-x", "hip", "--offload-device-only", "-S", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s: %s" % (src, r.stderr[-2000:]))
    return src, open(out).read(), r.stderr


def functions(asm):
    """-> {mangled name: normalised instruction text}, set of the names that are kernels"""
    out, cur, kernels = {}, None, set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    is_function = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, flags=re.M))      # (not the data tables)
    for ln in asm.splitlines():
        m = re.match(r"^(\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in is_function else None; continue
        if cur is None:
            continue
        s = ln.split(";", 1)[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None; continue
        if not s or (s.startswith(".") and not re.match(r"^\.L\w+:", s)):
            continue
        cur.append(re.sub(r"\.(LBB|Ltmp|LJTI|LCPI)\d+_", r".\1_", " ".join(s.split())))
    return {k: "\n".join(v) for k, v in out.items()}, kernels


def resources(remarks):
    rows, cur = {}, None
    for ln in remarks.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass", ln)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = rows.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1); cur[k.strip()] = v.strip()
    return rows


def side(csrc, jobs, keep, tag):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=max(1, min(16, jobs, len(srcs)))) as pool:
        done = list(pool.map(compile_unit, [(csrc, s, os.path.join(keep, "%s_%s.s" % (tag, os.path.splitext(s)[0]))) for s in srcs]))
    code, res, where, kernels = {}, {}, {}, set()
    for src, asm, remarks in done:
        fns, ks = functions(asm)
        kernels |= ks
        for name, text in fns.items():
            code.setdefault(name, set()).add(text)
            where.setdefault(name, []).append(src)
        for name, r in resources(remarks).items():
            res.setdefault(name, set()).add(tuple(sorted(r.items())))
    return code, res, where, kernels


def main():
    args = sys.argv[1:]
    opt = {"--csrc": os.path.join(ROOT, "miniweatherml_amd", "csrc"), "--base": None, "--jobs": "8", "--keep": None}
    renames = {}
    for i in range(0, len(args), 2):
        if i + 1 < len(args) and args[i] == "--rename" and "=" in args[i + 1]:
            old, new = args[i + 1].split("=", 1)
            renames[old] = new; continue
        if args[i] not in opt or i + 1 >= len(args):
            sys.exit(__doc__)
        opt[args[i]] = args[i + 1]
    if not opt["--base"]:
        sys.exit(__doc__)
    keep = opt["--keep"] or tempfile.mkdtemp(prefix="mw_devcmp_")
    os.makedirs(keep, exist_ok=True)
    b_code, b_res, b_where, b_k = side(opt["--base"], int(opt["--jobs"]), keep, "base")
    n_code, n_res, n_where, n_k = side(opt["--csrc"], int(opt["--jobs"]), keep, "new")
    for old, new in renames.items():
        if old not in b_code:
            sys.exit("--rename: the base has no function %s" % old)
        print("RENAMED: %s -> %s" % (old, new))
        for d in (b_code, b_res, b_where):
            if old in d:
                d[new] = d.pop(old)
        if old in b_k:
            b_k = (b_k - {old}) | {new}
    bad = 0
    for name in sorted(set(b_k) | set(n_k)):
        if name not in n_k or name not in b_k:
            print("ONLY IN %s: %s" % ("base" if name in b_k else "new", name)); bad += 1; continue
        for tag, where in (("base", b_where), ("new", n_where)):
            if len(where[name]) > 1:
                print("DEFINED TWICE in %s (%s): %s" % (tag, ", ".join(where[name]), name)); bad += 1
    same_code = same_res = 0
    for name in sorted(set(b_code) & set(n_code)):
        kind = "kernel" if name in n_k else "device function"
        if b_code[name] == n_code[name]:
            same_code += name in n_k
        else:
            print("CODE DIFFERS (%s; %s -> %s): %s" % (kind, ", ".join(b_where[name]), ", ".join(n_where[name]), name)); bad += 1
        if b_res.get(name) == n_res.get(name):
            same_res += name in n_k
        else:
            print("RESOURCES DIFFER (%s): %s\n  base %s\n  new  %s" % (kind, name, sorted(b_res.get(name, [])), sorted(n_res.get(name, [])))); bad += 1
    print("kernels: %d in base, %d in new; instruction streams equal: %d; resource lines equal: %d; findings: %d   (assembly kept in %s)" % (
        len(b_k), len(n_k), same_code, same_res, bad, keep))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
