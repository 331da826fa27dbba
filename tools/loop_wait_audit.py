"""Where do the loops of a unit's kernels wait for their global loads?  (no GPU needed)

    python tools/loop_wait_audit.py mw_march_xz.hip [mw_march_y.hip ...] [--filter SUBSTRING] [--asm FILE.s] [--strict]

vmcnt counts loads and stores and retires them in issue order (see landed() in csrc/mw_march.h): a marching loop issues a level's
loads at the top and is meant to wait for them once, as the counted vmcnt sequence in front of its stores.  A value that the compiler
consumes where it is declared puts an s_waitcnt vmcnt right behind the loads instead, and every level then pays a full memory round trip.
Nothing in the results shows that, and the source does not either; the device assembly does.

The tool compiles each unit to gfx950 assembly with the flags of miniweatherml_amd/build.py, into a temporary directory (the in-tree
objects are not touched; --asm reads an assembly file instead), and for every kernel and every loop (a backward branch to a block label)
whose body holds at least MIN_LOADS global loads prints
    the loads and stores of the body, its length in instructions, and per load  distance/count :
    the instruction distance from the load to the first s_waitcnt vmcnt behind it, and that wait's count.
A loop is FLAGGED when a vmcnt wait stands fewer than NEAR instructions behind a load that it waits for while at least MIN_LOADS loads
of the same iteration are outstanding (issued in this trip and not yet retired by an earlier wait of it): the wait's count says how many
of the operations in flight may stay in flight, and the ones it retires are the oldest.  A counted wait right behind a load that only
retires operations issued long before -- the pipelined form -- is what the design asks for and is not flagged.
Trips: one pass from the loop's head to its backward branch.  A wave-uniform forward branch (on SCC / VCC) is followed both ways, so that
the two forms of an iteration are not read as one; a branch on EXEC only skips predicated code and is read as not taken; backward
branches of inner loops fall through.  Distances count the instructions of the trip.  Stores of the previous iteration that are still in
flight at the loop's head are not counted (they make a wait retire more, never less).
--filter (may be repeated) keeps the kernels whose name holds every substring.  The tool reports; with --strict the exit status is 1 when
a loop of the kernels looked at is flagged (forms off the headline path are flagged as they stand: gate with a filter).
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "miniweatherml_amd", "csrc")
NEAR = 32            # a wait this close behind a load that it waits for ...
MIN_LOADS = 8        # ... with this many loads of the iteration in flight is exposed; also the smallest loop that is looked at
MAX_STATES = 200000  # states of one loop's trips that are followed before the tool gives up on the loop

_LOAD = re.compile(r"^(global|flat|buffer)_load")
_STORE = re.compile(r"^(global|flat|buffer)_(store|atomic)")
_WAIT = re.compile(r"^s_waitcnt\b.*\bvmcnt\((\d+)\)")
_BRANCH = re.compile(r"^(s_c?branch\w*)\s+(\.LBB\d+_\d+)")


def build_settings():
    """(hipcc, flags) of miniweatherml_amd/build.py, read from the file itself (importing the package would load the library)"""
    spec = importlib.util.spec_from_file_location("_mw_build", os.path.join(ROOT, "miniweatherml_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, [f for f in mod.FLAGS if not f.startswith("-W")]


def compile_unit(src):
    hipcc, flags = build_settings()
    with tempfile.TemporaryDirectory(prefix="mw_waitaudit_") as tmp:
        out = os.path.join(tmp, os.path.splitext(os.path.basename(src))[0] + ".s")
        cmd = [hipcc] + flags + ["-x", "hip", "--offload-device-only", "-S", src, "-o", out]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s: %s" % (src, r.stderr[-2000:]))
        return open(out).read()


def kernels(asm):
    """-> [(mangled name, [instruction or label, ...])] of the kernels of an assembly text, comments and directives stripped"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    out, cur = [], None
    for ln in asm.splitlines():
        m = re.match(r"^(\w+):", ln)
        if m:
            cur = None
            if m.group(1) in names:
                cur = []; out.append((m.group(1), cur))
            continue
        if cur is None:
            continue
        s = " ".join(ln.split(";", 1)[0].split())
        if s.startswith(".Lfunc_end"):
            cur = None; continue
        if not s or (s.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", s)):
            continue
        cur.append(s)
    return out


def loops(body):
    """-> (instructions, {label: index of its first instruction}, [(head label, first, last instruction)]): one loop per block label
    that a later branch jumps back to"""
    label_at, ins = {}, []
    for s in body:
        if s.endswith(":"):
            label_at[s[:-1]] = len(ins)
        else:
            ins.append(s)
    last = {}
    for i, s in enumerate(ins):
        m = _BRANCH.match(s)
        if m and m.group(2) in label_at and label_at[m.group(2)] <= i:
            last[m.group(2)] = max(last.get(m.group(2), 0), i)
    return ins, label_at, [(lab, label_at[lab], end) for lab, end in sorted(last.items(), key=lambda t: label_at[t[0]])]


def audit_loop(ins, label_at, first, last):
    """every trip through the loop body [first, last] -> dict, or None when the body holds fewer than MIN_LOADS loads.
    A trip's state: its memory operations that no wait has retired yet, oldest first, as (is_load, instruction, trip step of its issue)."""
    n_loads = sum(1 for s in ins[first:last + 1] if _LOAD.match(s))
    if n_loads < MIN_LOADS:
        return None
    n_stores = sum(1 for s in ins[first:last + 1] if _STORE.match(s))
    heads = set(label_at.values())
    first_wait, findings, seen, truncated = {}, {}, set(), False
    stack = [(first, 0, (), frozenset())]              # (instruction, trip step, in flight, loads that have not met a wait yet)
    while stack:
        i, step, inflight, unwaited = stack.pop()
        while True:
            if i in heads:
                # (two trips that reach a block with the same operations in flight, of the same age up to NEAR, go on alike)
                key = (i, tuple((l, at, min(step - t, NEAR)) for l, at, t in inflight), unwaited)
                if key in seen:
                    break
                seen.add(key)
                if len(seen) > MAX_STATES:
                    truncated = True; stack = []; break
            s = ins[i]
            m = _WAIT.match(s)
            if _LOAD.match(s):
                inflight = inflight + ((True, i, step),); unwaited = unwaited | {i}
            elif _STORE.match(s):
                inflight = inflight + ((False, i, step),)
            elif m:
                cnt = int(m.group(1))
                for l, at, t in inflight:
                    if at in unwaited and (at not in first_wait or step - t < first_wait[at][0]):
                        first_wait[at] = (step - t, cnt)
                unwaited = frozenset()
                retired = inflight[:max(len(inflight) - cnt, 0)]
                out_loads = sum(1 for l, _, _ in inflight if l)
                near = [step - t for l, _, t in retired if l and step - t < NEAR]
                if near and out_loads >= MIN_LOADS:
                    f = findings.setdefault(i, {"at": i - first, "vmcnt": cnt, "behind_load": min(near), "loads_outstanding": out_loads})
                    f["behind_load"] = min(f["behind_load"], min(near)); f["loads_outstanding"] = max(f["loads_outstanding"], out_loads)
                inflight = inflight[len(retired):]
            if i == last:
                break
            step += 1
            m = _BRANCH.match(s)
            if m and m.group(2) in label_at:
                t = label_at[m.group(2)]
                forward = i < t <= last
                if m.group(1) == "s_branch":
                    if not forward:
                        break                            # (leaves the loop)
                    i = t; continue
                if forward and "exec" not in m.group(1):   # a wave-uniform choice: both ways (a branch on EXEC only skips predicated code)
                    stack.append((t, step, inflight, unwaited))
            i += 1
    pairs = [first_wait[l] for l in sorted(first_wait)]
    return {"instructions": last - first + 1, "loads": n_loads, "stores": n_stores, "load_to_wait": pairs,
            "never_waited": n_loads - len(pairs), "findings": [findings[k] for k in sorted(findings)], "truncated": truncated}


def demangle(names):
    for tool in ("c++filt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            r = subprocess.run([tool] + names, capture_output=True, text=True)
            if r.returncode == 0:
                return [ln.split("(")[0].replace("void mw::", "") for ln in r.stdout.splitlines()]
        except OSError:
            pass
    return names


def audit_asm(asm, filt=()):
    """-> [{"kernel", "mangled", "loop", ...audit_loop()}] for the loops of the kernels whose demangled name holds every filter string"""
    ks = kernels(asm)
    nice = demangle([k for k, _ in ks]) if ks else []
    rows = []
    for (mangled, body), name in zip(ks, nice):
        if any(f not in name for f in filt):
            continue
        ins, label_at, found = loops(body)
        for lab, first, last in found:
            a = audit_loop(ins, label_at, first, last)
            if a:
                a.update(kernel=name, mangled=mangled, loop=lab)
                rows.append(a)
    return rows


def audit_unit(src, filt=()):
    return audit_asm(compile_unit(src), filt)


def report(unit, rows, out=sys.stdout):
    flagged = 0
    out.write("== %s: %d loops with >= %d global loads\n" % (unit, len(rows), MIN_LOADS))
    for r in rows:
        d = r["load_to_wait"]
        near = min((p[0] for p in d), default=None)
        out.write("%s %s  loop %s: %d instructions, %d loads, %d stores; first wait behind a load: nearest %s%s\n" % (
            "FLAGGED" if r["findings"] else "ok     ", r["kernel"], r["loop"], r["instructions"], r["loads"], r["stores"], near,
            "  (more than %d states: not every trip was read)" % MAX_STATES if r["truncated"] else ""))
        out.write("    load -> first vmcnt wait, distance/count: %s%s\n" % (
            " ".join("%d/%d" % p for p in d), ("  (+%d loads met by no wait of the body)" % r["never_waited"]) if r["never_waited"] else ""))
        for f in r["findings"]:
            flagged += 1
            out.write("    ** s_waitcnt vmcnt(%d) at instruction %d, %d behind a load, %d loads of the iteration outstanding\n" % (
                f["vmcnt"], f["at"], f["behind_load"], f["loads_outstanding"]))
    return flagged


def main():
    args, units, filt, asm_file, strict = sys.argv[1:], [], [], None, False
    while args:
        a = args.pop(0)
        if a == "--filter" and args:
            filt.append(args.pop(0))
        elif a == "--strict":
            strict = True
        elif a == "--asm" and args:
            asm_file = args.pop(0)
        elif a.endswith(".hip"):
            units.append(a)
        else:
            sys.exit(__doc__)
    if not units and not asm_file:
        sys.exit(__doc__)
    flagged = 0
    if asm_file:
        flagged += report(os.path.basename(asm_file), audit_asm(open(asm_file).read(), filt))
    for u in units:
        flagged += report(u, audit_unit(u, filt))
    print("flagged waits: %d" % flagged)
    sys.exit(1 if flagged and strict else 0)


if __name__ == "__main__":
    main()
