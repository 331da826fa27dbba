"""Shared helpers for the parity tests (tests only)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Every compare_fields() call appends what it OBSERVED (max|diff| / scale per field, the limit it was held to, and whether the
# sensitivity fallback was needed) to this JSON-lines file; tests/conftest.py condenses it into parity_r<NN>.json at session end
# and the round's copy is committed under profiles/.
PARITY_LOG = os.environ.get("MW_PARITY_LOG", os.path.join(ROOT, "gpurun_out", "parity_observed.jsonl"))

# The ONLY cases that may use the `10 x oracle 1-ulp sensitivity` fallback: the thermal bubble -- whose
# saturated core sits on the reference algorithm's branch discontinuities (convexify's `tot > 1e-20`, the upwind selector) so
# that the ORACLE run from inputs one ulp apart diverges by up to 1e-8 after a step -- and the wall/open boundary tests built
# on that case.  Everything else is held to the plain 1e-11 / 1e-9 (1e-10 for 2-5 steps) of BASELINE.md section 4.
SENS_ALLOW = ("thermal3d_16x16x16", "bc ", "zperiodic")


def sens_allowed(what):
    return any(what.startswith(a) for a in SENS_ALLOW)


def set_options(monkeypatch, **opts):
    """Run-time options (mw_dycore_set_option) for every dycore handle created from here to the end of the test: the typed replacement
    of the MW_* environment switches of rounds 1-4 (modules.DEFAULT_OPTIONS is applied right after mw_dycore_create)."""
    from miniweatherml_amd import modules
    for k, v in opts.items():
        monkeypatch.setitem(modules.DEFAULT_OPTIONS, k, int(v))


def launched_kernels(reset=True):
    """Mangled names of the dycore kernels this process has launched since the last reset (mw_debug_launched_kernels)."""
    from miniweatherml_amd import capi
    L = capi.lib()
    n = L.mw_debug_launched_kernels(None, 0, 0)
    buf = C.create_string_buffer(int(n) + 16)
    L.mw_debug_launched_kernels(buf, len(buf), 1 if reset else 0)
    return sorted(set(buf.value.decode().split()))


def kernel_forms(names):
    """Mangled kernel names (launched_kernels) -> {kernel family: set of template-argument tuples}: the integral and bool arguments
    of every instantiation in declaration order, e.g. k_xz_state<1, true, 0, 1, 1, 5, false, true> -> (1, 1, 0, 1, 1, 5, 0, 1)."""
    import re
    out = {}
    for n in names:
        m = re.match(r"_ZN2mw(\d+)", n)
        if not m:
            continue
        ln, at = int(m.group(1)), m.end()
        family, rest = n[at:at + ln], n[at + ln:]
        args = []
        if rest.startswith("I"):
            at = 1
            while True:
                a = re.match(r"L[ib](n?)(\d+)E", rest[at:])
                if not a:
                    break
                args.append(-int(a.group(2)) if a.group(1) else int(a.group(2)))
                at += a.end()
        out.setdefault(family, set()).add(tuple(args))
    return out


def zero_row_maps(dycore):
    """The ten zero-row maps of the handle's last sub-cycle (mw_debug_zero_maps): uint32 (10, nz, ny + 18) -- M0, Q1 .. Q3, FN1 .. FN3,
    QY1 .. QY3, row j at column j + 9; None when the sub-cycle ran without maps (or the handle keeps one set per member)."""
    from miniweatherml_amd import capi
    L, dims = capi.lib(), (C.c_int * 2)()
    n = L.mw_debug_zero_maps(dycore.h, None, 0, dims)
    if n <= 0:
        return None
    buf = np.zeros(n, dtype=np.uint32)
    assert L.mw_debug_zero_maps(dycore.h, buf.ctypes.data_as(C.c_void_p), n, dims) == n
    return buf.reshape(10, dims[0], dims[1])


def zero_row_seg_mask(lo, hi, nxi):
    """The segment bits (in place: bits 4 .. 29) of the cells lo .. hi of a PERIODIC row of nxi cells, lo may be < 0 and hi >= nxi
    (26 segments of ceil(nxi / 26) cells)."""
    L = (nxi + 25) // 26
    span = lambda a, b: ((2 << (b // L)) - (1 << (a // L))) << 4   # noqa: E731
    if hi - lo + 1 >= nxi:
        return span(0, nxi - 1)
    if lo < 0:
        return span(lo + nxi, nxi - 1) | span(0, hi)
    if hi >= nxi:
        return span(lo, nxi - 1) | span(0, hi - nxi)
    return span(lo, hi)


def drain_paths():
    """The dispatcher paths (mw_dycore_path) of every time_step since the last drain."""
    from miniweatherml_amd import modules
    p = sorted(set(modules.PATH_LOG))
    modules.PATH_LOG.clear()
    return p


def rel_err(a, b):
    """max|a-b| / max|b|  (the tolerance definition of BASELINE.md section 4)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = np.max(np.abs(b))
    d = np.max(np.abs(a - b))
    return d / scale if scale > 0 else d


def gpu_fields(coupler):
    """coupler fields -> dict of numpy arrays, oracle naming (tracer0..)."""
    dm = coupler.get_data_manager_readonly()
    out = {n: dm.get(n, True).cpu().numpy() for n in ("density_dry", "uvel", "vvel", "wvel", "temp")}
    for t, n in enumerate(coupler.get_tracer_names()):
        out["tracer%d" % t] = dm.get(n, True).cpu().numpy()
    return out


def push_fields(coupler, f):
    """oracle Fields -> coupler tensors (identical inputs on both sides)."""
    import torch
    dm = coupler.get_data_manager_readwrite()
    for n, a in (("density_dry", f.rho_d), ("uvel", f.uvel), ("vvel", f.vvel), ("wvel", f.wvel), ("temp", f.temp)):
        dm.get(n).copy_(torch.from_numpy(a))
    for t, n in enumerate(coupler.get_tracer_names()):
        dm.get(n).copy_(torch.from_numpy(f.tracers[t]))


# absolute floor for fields that are identically ~0 in the oracle (e.g. vvel early in a symmetric run)
ABS_FLOOR = {"vvel": 1e-11, "wvel": 1e-11, "uvel": 1e-11, "tracer1": 1e-14, "tracer2": 1e-14}


_LIBM_OK = None


def host_libm_matches_restatement():
    """The strict forms carry glibc's pow / exp as built for FMA-capable x86-64 hosts (csrc/mw_glibc_pow.h restates the __pow_fma /
    __exp_fma / __cos_fma builds of glibc 2.35, Ubuntu 22.04's libm.so.6 -- DESIGN.md section 2).  On a host whose libm resolves to
    another build (no FMA: the ifunc picks the SSE2 variant, which rounds a few intermediate products differently; or another glibc
    release) the CPU oracle itself computes slightly different bits and bit-equality cannot be asked for.  That must never pass
    silently as "bitwise": the check FAILS the comparison that asked for bit-equality (round 4; it used to warn and fall back to a
    tolerance).  MW_ALLOW_LIBM_MISMATCH=1 restores the tolerance fallback for a deliberate run on such a host.
    Checked once per session on 2e5 arguments."""
    global _LIBM_OK
    if _LIBM_OK is None:
        import warnings
        from oracle import mw_oracle
        libm_pow, restated = mw_oracle.powcheck()
        rng = np.random.default_rng(99)
        x, y = rng.uniform(1e-3, 5e2, 200_000), rng.uniform(0.3, 3.6, 200_000)
        got, main = restated(x, y)
        _LIBM_OK = bool(np.array_equal(libm_pow(x, y)[main].view(np.uint64), got[main].view(np.uint64)))
        if not _LIBM_OK:
            warnings.warn("host libm's pow is not the build csrc/mw_glibc_pow.h restates")
    if not _LIBM_OK:
        import os
        if os.environ.get("MW_ALLOW_LIBM_MISMATCH") != "1":
            raise AssertionError("host libm's pow is not the build csrc/mw_glibc_pow.h restates (glibc 2.35, x86-64 FMA variants): the strict "
                                 "path cannot be held to bit-equality with the CPU oracle on this host -- set MW_ALLOW_LIBM_MISMATCH=1 to "
                                 "compare with tolerances instead")
    return _LIBM_OK


def compare_fields(got, ref, tol, what="", sens=None):
    """tol: relative to max|field|.  sens: optional per-field absolute sensitivity of the
    reference ALGORITHM itself to a 1-ulp input perturbation (oracle_sensitivity below); the limit is then
    max(tol*scale, 10*sens): an implementation cannot be asked to track the oracle more closely than the oracle tracks
    itself across the algorithm's own branch discontinuities (`if (tot > 1.e-20)` in convexify,
    WenoLimiter_recon.h:12-15, and the upwind selector `ind = (m_L + m_R > 0) ? 0 : 1`, :408)."""
    if sens is not None and not sens_allowed(what):
        raise AssertionError("%s: the sensitivity fallback is reserved for the allow-listed cases %r" % (what, SENS_ALLOW))
    # The STRICT kernel path ("mode 1": the reference's operation order, contraction off, glibc's pow -- csrc/mw_glibc_pow.h) is held
    # to BIT-EQUALITY with the oracle: no tolerance, no floor, no sensitivity fallback (round 3).
    bitwise = " mode 1" in what and host_libm_matches_restatement()
    if bitwise:
        sens = None
    elif " mode 1" in what and tol == 0.0:
        tol = 1e-13                                            # (a host whose libm is not the restated build: see below)
    worst, rec, fail = {}, {}, None
    for k in ref:
        scale = float(np.max(np.abs(ref[k])))
        d = float(np.max(np.abs(got[k] - ref[k])))
        plain = 0.0 if bitwise else tol * scale + ABS_FLOOR.get(k, 0.0) * (tol / 1e-11)
        lim = plain
        if sens is not None:
            lim = max(lim, 10.0 * sens[k])
        if bitwise and fail is None and not np.array_equal(got[k], ref[k]):
            fail = "%s: field %s is not bit-identical to the oracle (max|diff| %.3e, scale %.3e)" % (what, k, d, scale)
        worst[k] = (d, scale)
        rec[k] = {"max_abs_diff": d, "scale": scale, "rel": (d / scale if scale > 0 else d), "limit_abs": lim,
                  "needed_fallback": bool(d > plain)}
        if fail is None and not np.all(np.isfinite(got[k])):
            fail = "%s: non-finite values in %s" % (what, k)
        if fail is None and not d <= lim:
            fail = "%s: field %s max|diff| %.3e > %.3e (scale %.3e)" % (what, k, d, lim, scale)
    try:
        paths, kernels = drain_paths(), launched_kernels(reset=True)       # what produced the compared fields (GPU side)
    except Exception:                                              # (CPU-only sessions: oracle against golden vectors, no library call)
        paths, kernels = [], []
    try:
        os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
        with open(PARITY_LOG, "a") as fh:
            fh.write(json.dumps({"what": what, "tol": 0.0 if bitwise else tol, "bitwise": bitwise, "fallback_allowed": sens is not None, "passed": fail is None,
                                 "test": os.environ.get("PYTEST_CURRENT_TEST", ""), "paths": paths, "kernels": kernels, "fields": rec}) + "\n")
    except OSError:
        pass
    assert fail is None, fail
    return worst
ABS_FLOOR.update({"tracer%d" % t: 1e-14 for t in range(3, 16)})


_SENS_CACHE = {}


def oracle_sensitivity(oracle, key, make, steps):
    """Runs the CPU oracle twice from inputs that differ by ONE ULP in `temp` (random sign per cell) and returns
    {step: {field: max|difference|}} for the requested step counts.  `make()` -> (OracleDycore, Fields)."""
    key = (key, tuple(steps))
    if key in _SENS_CACHE:
        return _SENS_CACHE[key]
    d1, f1 = make()
    d2, f2 = make()
    rng = np.random.default_rng(1234)
    f2.temp *= (1.0 + np.sign(rng.normal(size=f2.temp.shape)) * 2.0 ** -52)
    dt = d1.compute_time_step()
    out = {}
    for s in range(1, max(steps) + 1):
        d1.time_step(f1, dt)
        d2.time_step(f2, dt)
        if s in steps:
            a, b = f1.as_dict(), f2.as_dict()
            out[s] = {k: float(np.max(np.abs(a[k] - b[k]))) for k in a}
    _SENS_CACHE[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------------
# In-process rank emulation (threads): R product handles on one GPU / R oracle ranks on the CPU
# ------------------------------------------------------------------------------------------------------------------
import ctypes as C      # noqa: E402
import threading        # noqa: E402


class Exchanger:
    """All ranks live in this process; strips are copied device-to-device after a barrier."""

    def __init__(self, nranks):
        self.n = nranks
        self.bar = threading.Barrier(nranks)
        self.send = [None] * nranks
        self.errors = []

    def make_cb(self, rank, grid):
        from miniweatherml_amd import capi
        peers, so, ro, act = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
        capi.check(capi.lib().mw_exchange_plan(C.byref(grid), peers, so, ro, act))
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]

        def cb(ctx, sW, sE, sS, sN, rW, rE, rS, rN, nWE, nSN, stream):
            try:
                hip.hipStreamSynchronize(stream)                          # my strips are packed
                self.send[rank] = (sW, sE, sS, sN)
                self.bar.wait(timeout=60)
                cnt = [nWE, nWE, nSN, nSN]
                recv = [rW, rE, rS, rN]
                for d in range(4):                                      # my halo d comes from peer[d]'s opposite strip
                    if recv[d] and cnt[d] and act[d]:
                        src = self.send[peers[d]][d ^ 1]
                        assert hip.hipMemcpy(recv[d], src, cnt[d] * 8, 3) == 0      # hipMemcpyDeviceToDevice
                # a device-to-device hipMemcpy is not synchronous with the host, and the library's streams do not synchronise
                # with the null stream it runs on: finish the copies before the unpack kernels are enqueued
                assert hip.hipStreamSynchronize(None) == 0
                self.bar.wait(timeout=60)
                return 0
            except Exception as e:                                      # pragma: no cover
                self.errors.append(repr(e))
                self.bar.abort()
                return 1
        return capi.EXCHANGE_FN(cb)



class OracleExchanger:
    """The oracle's halo/edge exchange callback between oracle ranks living in threads of this process."""

    def __init__(self, nranks, plans):
        self.n, self.plans = nranks, plans
        self.bar = threading.Barrier(nranks)
        self.send = [None] * nranks

    def make_cb(self, rank):
        peers, act = self.plans[rank]

        def cb(ctx, kind, sW, sE, sS, sN, rW, rE, rS, rN, nWE, nSN):
            cnt = [nWE, nWE, nSN, nSN]
            sb, rb = [sW, sE, sS, sN], [rW, rE, rS, rN]
            self.send[rank] = [np.ctypeslib.as_array(sb[d], shape=(cnt[d],)).copy() if cnt[d] else None for d in range(4)]
            self.bar.wait(timeout=120)
            for d in range(4):
                if cnt[d]:
                    src = self.send[peers[d]][d ^ 1] if act[d] else self.send[rank][d ^ 1]      # single rank in a direction: self wrap
                    np.ctypeslib.as_array(rb[d], shape=(cnt[d],))[:] = src
            self.bar.wait(timeout=120)
        return cb




class StreamExchanger:
    """Stream-ordered in-process transport (round 5): like Exchanger, all ranks live in threads of this process and strips are copied
    device-to-device, but NOTHING waits on the host for the device inside the callback -- the copies run on a per-rank side stream behind
    the peers' post-pack events, and the caller's stream waits for events, exactly the shape of the built-in RCCL transport
    (mw_rccl.cpp: ev_ready -> side stream -> ev_done).  The two host barriers only hand event / buffer handles from thread to thread.
    fuzz_seed != 0: spin kernels of seeded random length (mw_debug_spin) in front of and behind the copies, so that a missing wait in the
    schedule shows up as a wrong bit instead of hiding behind lucky timing."""

    def __init__(self, nranks, fuzz_seed=0):
        import torch                                               # noqa: F401  (the HIP runtime torch loaded is the process's one)
        self.n = nranks
        self.bar = threading.Barrier(nranks)
        self.send = [None] * nranks
        self.errors = []
        self.fuzz = fuzz_seed
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipEventCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
        hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        hip.hipEventDestroy.argtypes = [C.c_void_p]
        self.hip = hip
        self.lanes = {}                                            # (rank, caller stream) -> (side stream, ready event, copied event)
        self.ready = [None] * nranks
        self.copied = [None] * nranks
        self.calls = 0

    def close(self):
        """Side streams and events of this transport (call when every rank has finished and synchronised)."""
        for side, e0, e1 in self.lanes.values():
            self.hip.hipStreamSynchronize(side)
            self.hip.hipEventDestroy(e0)
            self.hip.hipEventDestroy(e1)
            self.hip.hipStreamDestroy(side)
        self.lanes = {}

    def _lane(self, rank, stream):
        key = (rank, stream or 0)
        if key not in self.lanes:
            side, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert self.hip.hipStreamCreateWithFlags(C.byref(side), 1) == 0                 # hipStreamNonBlocking
            assert self.hip.hipEventCreateWithFlags(C.byref(e0), 2) == 0                    # hipEventDisableTiming
            assert self.hip.hipEventCreateWithFlags(C.byref(e1), 2) == 0
            self.lanes[key] = (side, e0, e1)
        return self.lanes[key]

    def make_cb(self, rank, grid):
        from miniweatherml_amd import capi
        L = capi.lib()
        peers, so, ro, act = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
        capi.check(L.mw_exchange_plan(C.byref(grid), peers, so, ro, act))
        hip = self.hip
        rng = np.random.default_rng([self.fuzz, rank]) if self.fuzz else None

        def spin(stream):
            if rng is not None:
                us = int(rng.integers(0, 250))
                if us:
                    capi.check(L.mw_debug_spin(us, stream))

        def cb(ctx, sW, sE, sS, sN, rW, rE, rS, rN, nWE, nSN, stream):
            try:
                side, ready, copied = self._lane(rank, stream)
                assert hip.hipEventRecord(ready, stream) == 0             # my strips are packed (and my last unpack has read its buffers)
                self.send[rank] = (sW, sE, sS, sN)
                self.ready[rank], self.copied[rank] = ready, copied
                self.bar.wait(timeout=120)                               # (host rendezvous: handles only)
                cnt = [nWE, nWE, nSN, nSN]
                recv = [rW, rE, rS, rN]
                assert hip.hipStreamWaitEvent(side, ready, 0) == 0
                spin(side)
                for d in range(4):                                      # my halo d comes from peer[d]'s opposite strip
                    if recv[d] and cnt[d] and act[d]:
                        assert hip.hipStreamWaitEvent(side, self.ready[peers[d]], 0) == 0
                        src = self.send[peers[d]][d ^ 1]
                        assert hip.hipMemcpyAsync(recv[d], src, cnt[d] * 8, 3, side) == 0      # hipMemcpyDeviceToDevice
                spin(side)
                assert hip.hipEventRecord(copied, side) == 0
                self.bar.wait(timeout=120)                               # every rank's `copied` event has been recorded
                assert hip.hipStreamWaitEvent(stream, copied, 0) == 0     # my halos have arrived ...
                for d in range(4):                                      # ... and the peers have read my strips: the buffers may be packed again
                    if act[d] and cnt[d]:
                        assert hip.hipStreamWaitEvent(stream, self.copied[peers[d]], 0) == 0
                self.bar.wait(timeout=120)                               # (nobody re-records an event a peer is still about to wait for)
                return 0
            except Exception as e:                                      # pragma: no cover
                self.errors.append(repr(e))
                self.bar.abort()
                return 1
        return capi.EXCHANGE_FN(cb)


# ------------------------------------------------------------------------------------------------------------------
# The dispatcher's path space (round 5): every combination of kernel family x folded configuration x WENO order x internal layout x
# schedule x y launch form x where D1 happens x tracer stage x 2-D / 3-D x transport that mw_dycore_time_step can choose -- a Python
# statement of its rules (mw_dycore.hip: march / y_all_ok / marching_config / member_major / pipe_conv / conv_pending), spelled like
# mw_dycore_path spells them.  tests/test_gpu_path_matrix.py realises each one against the oracle; tests/conftest.py asserts at session
# end that every one was hit by a passed oracle comparison and that the library never reported a path outside this set.
# ------------------------------------------------------------------------------------------------------------------
def path_string(c):
    if c["family"] != "march":
        return "%s ord%d %s%s" % (c["family"], c["ord"], c["layout"], " transport" if c["transport"] else "")
    return "march ord%d K%d %s %s %s %s %s %s%s" % (c["ord"], c["K"], c["layout"], c["sched"], c["y"], c["conv"], c["tracers"], c["dim"],
                                                    " transport" if c["transport"] else "")


def path_valid(c):
    """The dispatcher's rules (see above).  fused_members = nens > 1 in the coupler's member-fastest layout (option member_major = 0)."""
    o, K, lay, sch, y, cv, tr, dim, tp = c["ord"], c["K"], c["layout"], c["sched"], c["y"], c["conv"], c["tracers"], c["dim"], c["transport"]
    if lay == "fused_members" and (o != 5 or K != 0):
        return False                                              # WENO-3 marches member-major only; a folded configuration needs a one-member view
    if lay in ("member_major", "mm_direct") and tr != "tracers_fused":
        return False                                              # member-major exists for the fused tracer stage
    if o == 3 and tr != "tracers_fused":
        return False
    if dim == "2d" and (K != 0 or y != "y_split" or cv != "conv_pass" or sch == "pipe"):
        return False                                              # 2-D: no y launch, no row wrap, never a folded configuration
    if y == "y_all" and (tr != "tracers_fused" or sch == "two_stream"):
        return False
    if sch == "pipe" and (y != "y_all" or not tp):
        return False
    if cv == "conv_pipe" and not (sch == "pipe" and (lay in ("nens1", "fused_members") or (lay == "mm_direct" and K != 0))):
        return False
    if cv == "conv_in_y" and (sch == "pipe" or tp):
        return False                                              # needs both index wraps: a block of a decomposed domain has neither
    return True


def reachable_paths():
    out = []
    for fam in ("general-strict", "general-fast"):
        for o in (3, 5, 7, 9):
            for lay in ("nens1", "fused_members"):
                for tp in (False, True):
                    out.append(dict(family=fam, ord=o, layout=lay, transport=tp))
    for o in (3, 5):
        for K in (0, 1, 2):
            for lay in ("nens1", "fused_members", "member_major", "mm_direct"):
                for sch in ("one_stream", "two_stream", "pipe"):
                    for y in ("y_all", "y_split"):
                        for cv in ("conv_in_y", "conv_pipe", "conv_pass"):
                            for tr in ("tracers_fused", "tracers_unfused"):
                                for dim in ("3d", "2d"):
                                    for tp in (False, True):
                                        c = dict(family="march", ord=o, K=K, layout=lay, sched=sch, y=y, conv=cv, tracers=tr, dim=dim, transport=tp)
                                        if path_valid(c):
                                            out.append(c)
    return out


def record_comparison(what, passed=True):
    """For checks that do not go through compare_fields (flux arrays judged per variable over the three directions, bitwise array
    comparisons): logs the comparison with the dispatcher paths and kernel instantiations that produced the compared data, so that the
    session's coverage matrix (tests/conftest.py) credits them."""
    try:
        paths, kernels = drain_paths(), launched_kernels(reset=True)
        os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
        with open(PARITY_LOG, "a") as fh:
            fh.write(json.dumps({"what": what, "tol": None, "bitwise": False, "fallback_allowed": False, "passed": bool(passed),
                                 "test": os.environ.get("PYTEST_CURRENT_TEST", ""), "paths": paths, "kernels": kernels, "fields": {}}) + "\n")
    except Exception:
        pass
