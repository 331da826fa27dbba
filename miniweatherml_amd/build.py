"""Builds libmw_cdna4.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

    python -m miniweatherml_amd.build [--force]

hipcc cross-compiles without a GPU; the built .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmw_cdna4.so")
# the dycore is eight units (map: csrc/mw_dycore_int.h); every kernel family is launched from exactly one of them
SOURCES = ["mw_host.cpp", "mw_dycore.hip", "mw_march_y.hip", "mw_march_xz.hip", "mw_march_tracers.hip", "mw_march_sched.hip", "mw_zero_rows.hip",
           "mw_dycore_init.hip", "mw_dycore_aids.hip", "mw_kessler.hip", "mw_mlp.hip", "mw_surrogate_bank.hip", "mw_surrogate_eval_domain.hip", "mw_member.hip", "mw_member_sample.hip", "mw_member_guard.hip", "mw_member_water.hip", "mw_member_heat.hip", "mw_train.hip", "mw_column.hip", "mw_output.hip", "mw_netcdf.cpp", "mw_rccl.cpp", "mw_h5.cpp"]
HEADERS = ["mw_common.h", "mw_dycore_int.h", "mw_weno.h", "mw_weno79.h", "mw_march.h", "mw_zero_rows.h", "mw_calib.h", "mw_glibc_pow.h", "mw_glibc_pow_tables.h", "mw_kessler_teacher.h", "mw_sample_key.h", "mw_mlp_net.h", "mw_surrogate_bank.h", "mw_member.h", os.path.join("..", "..", "include", "mw_cdna4.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_JOBS = 16      # hipcc processes at a time (never sized by the machine's CPU count: build boxes are shared)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-ffp-contract=on", "-I/opt/rocm/include"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _depfile_headers(depfile):
    """The prerequisites a compile recorded in its depfile (-MMD -MF, make syntax, paths relative to csrc); None without one."""
    if not os.path.exists(depfile):
        return None
    words = open(depfile).read().replace("\\\n", " ").split()
    return [os.path.join(CSRC, w) for w in words[1:] if not w.endswith(":")]


def build(force=False, verbose=True):
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, cmds = [], []
    for s in srcs:
        stem = os.path.splitext(s)[0]
        o = os.path.join(CSRC, stem + ".o")
        objs.append(o)
        # stale: the source or a header it really includes is newer (the last compile's depfile); without a depfile, any of HEADERS
        deps = _depfile_headers(os.path.join(CSRC, stem + ".d"))
        if force or _stale(o, [os.path.join(CSRC, s)] + (hdrs if deps is None else deps)):
            # relative paths, run in csrc: the depfile stays valid in another checkout
            cmds.append([HIPCC] + FLAGS + (["-x", "hip"] if s.endswith(".hip") else []) + ["-MMD", "-MF", stem + ".d", "-c", s, "-o", stem + ".o"])

    def compile_one(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)

    if cmds:
        with ThreadPoolExecutor(max_workers=min(MAX_JOBS, len(cmds))) as pool:
            list(pool.map(compile_one, cmds))
    if force or _stale(LIB, objs):
        # RCCL is NOT linked: mw_rccl.cpp resolves it at run time from the librccl already mapped in the process (one RCCL)
        cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


def build_examples(verbose=True):
    """The C++ callers of examples/ (mirrors of the reference's drivers) against the C++ facade + C ABI."""
    root = os.path.dirname(HERE)
    exes = []
    for name in ("supercell_driver", "simple_city_driver", "inference_ponni_driver", "supercell_multirank"):
        src = os.path.join(root, "examples", name + ".cpp")
        exe = os.path.join(root, "examples", name)
        deps = [src, os.path.join(HERE, "host", "mw_facade.h"), os.path.join(HERE, "host", "mw_ponni.h"), os.path.join(root, "include", "mw_cdna4.h"), LIB]
        if _stale(exe, deps):
            cmd = [HIPCC, "-O2", "-std=c++17", "-x", "c++", src, "-o", exe, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                   "-L" + HERE, "-lmw_cdna4", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../miniweatherml_amd",
                   "-Wl,-rpath,/opt/rocm/lib"]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        exes.append(exe)
    # a module with its own HIP kernels over core::MultiField (MultipleFields.h:10-96): compiled as HIP for gfx950
    src = os.path.join(root, "examples", "multifield_module.cpp")
    exe = os.path.join(root, "examples", "multifield_module")
    if _stale(exe, [src, os.path.join(HERE, "host", "mw_facade.h"), os.path.join(root, "include", "mw_cdna4.h"), LIB]):
        cmd = [HIPCC, "-O2", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", src, "-o", exe, "-I/opt/rocm/include", "-L" + HERE, "-lmw_cdna4",
               "-Wl,-rpath,$ORIGIN/../miniweatherml_amd", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    exes.append(exe)
    return exes[0]


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_examples()
