"""Transports of a multi-rank run: the halo exchange of the dycore (halo_exchange, model/modules/dynamics_euler_stratified_wenofv.h:641-723,
its MPI_Isend / Irecv and the host-staged mode :687-722) over RCCL inside the library or torch.distributed point-to-point, and the sum over
ranks that the column modules' horizontal means need (MPI_Allreduce in sponge_layer.h / column_nudging.h)."""
import ctypes as C

import torch

from . import capi
from .capi import MWError, check


def install_exchange(dycore, coupler, transport="rccl", group=None):
    """Picks the halo-exchange transport for a multi-rank run TOGETHER on all ranks: the built-in RCCL transport unless any
    rank cannot set it up, in which case every rank switches to the torch.distributed point-to-point transport (ranks on
    different transports would deadlock).  Returns the transport in use: "none" (one rank), "rccl" or "torch"."""
    import torch.distributed as dist
    if coupler.get_nranks() <= 1:
        return "none"
    dev = coupler.device if dist.get_backend(group) != "gloo" else "cpu"

    def any_rank(failed):
        flag = torch.tensor([1 if failed else 0], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
        return int(flag.item()) == 1

    if transport == "rccl":
        failed, why = False, ""
        if not capi.lib().mw_rccl_library_path(None):                        # checked BEFORE the collective communicator set-up
            failed, why = True, "no librccl available to libmw_cdna4"
        if any_rank(failed):
            transport = "torch"
        else:
            try:
                use_rccl_exchange(dycore, coupler, group)
            except MWError as e:
                failed, why = True, str(e)
            if any_rank(failed):
                transport = "torch"
        if failed:
            import sys
            print("rank %d: built-in RCCL transport unavailable (%s)" % (coupler.get_myrank(), why), file=sys.stderr)
    if transport == "torch":
        use_torch_distributed_exchange(dycore, coupler, group)                # replaces (and frees) a half-installed RCCL transport
    return transport


def use_rccl_exchange(dycore, coupler, group=None):
    """Slab halo exchange over RCCL point-to-point inside the library (mw_rccl.cpp): rank 0 creates the ncclUniqueId,
    torch.distributed broadcasts it, every rank joins.  Replaces the MPI_Isend/Irecv of halo_exchange (:641-723)."""
    import torch.distributed as dist
    L = capi.lib()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    # 128 id bytes + 1 status byte.  Rank 0 ALWAYS reaches the broadcast -- with status 1 and a zero id when it could not create the
    # id -- and every rank raises only after it: a rank that left before the collective would leave the others waiting in it.
    ident = torch.zeros(129, dtype=torch.uint8, device=coupler.device)
    why = ""
    if rank == 0:
        buf = C.create_string_buffer(128)
        if L.mw_rccl_unique_id(buf) != 0:
            why = L.mw_last_error().decode(errors="replace")
            ident[128] = 1
        else:
            ident[:128].copy_(torch.tensor(list(buf.raw), dtype=torch.uint8))
    dist.broadcast(ident, 0, group=group)
    host = ident.cpu().tolist()
    if host[128]:
        raise MWError("rank 0 could not create the ncclUniqueId" + (": " + why if why else ""))
    with torch.cuda.device(coupler.device):
        check(L.mw_dycore_use_rccl(dycore.h, bytes(host[:128]), world, rank))


def use_rccl_self_exchange(dycore, coupler):
    """The self-loop test transport (mw_dycore_use_rccl_self): this one rank plays every rank of the coupler's rank grid over a 1-rank
    RCCL communicator -- the real send / receive groups on the side stream(s), on one GPU.  The column modules' sums go through the
    handle's communicator too (times the number of blocks)."""
    with torch.cuda.device(coupler.device):
        check(capi.lib().mw_dycore_use_rccl_self(dycore.h))
    use_rccl_allreduce(coupler, dycore)


def use_torch_distributed_exchange(dycore, coupler, group=None, host_staged=False):
    """Alternative transport for the same exchange: torch.distributed point-to-point ops (backend "nccl" = RCCL) issued
    from the library's exchange callback in the order of mw_exchange_plan.  Same wire pattern as the built-in transport.
    host_staged=True copies the strips through host buffers first -- the reference's non-GPU-aware-MPI mode
    (dynamics_euler_stratified_wenofv.h:687-722); works with the gloo backend."""
    import torch.distributed as dist
    L = capi.lib()
    peers, so, ro, act = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    check(L.mw_exchange_plan(C.byref(coupler.grid), peers, so, ro, act))
    dev = coupler.device

    def wrap(ptr, n):
        class _A:
            pass
        a = _A()
        a.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f8", data=(int(ptr), False), version=2)
        return torch.as_tensor(a, device=dev)

    def cb(ctx, sW, sE, sS, sN, rW, rE, rS, rN, nWE, nSN, stream):
        try:
            st = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
            with torch.cuda.device(dev), torch.cuda.stream(st):
                sb, rb, cnt = [sW, sE, sS, sN], [rW, rE, rS, rN], [nWE, nWE, nSN, nSN]
                if host_staged:
                    hs = {d: wrap(sb[d], cnt[d]).cpu() for d in range(4) if act[d] and cnt[d] and sb[d]}     # syncs the stream
                    hr = {d: torch.empty(cnt[d], dtype=torch.float64) for d in range(4) if act[d] and cnt[d] and rb[d]}
                    reqs = [dist.isend(hs[so[o]], peers[so[o]], group=group) for o in range(4) if so[o] in hs]
                    reqs += [dist.irecv(hr[ro[o]], peers[ro[o]], group=group) for o in range(4) if ro[o] in hr]
                    for r in reqs:
                        r.wait()
                    for d, t in hr.items():
                        wrap(rb[d], cnt[d]).copy_(t, non_blocking=False)
                    return 0
                ops = []
                for o in range(4):
                    d = so[o]
                    if act[d] and cnt[d] and sb[d]:
                        ops.append(dist.P2POp(dist.isend, wrap(sb[d], cnt[d]), peers[d], group))
                for o in range(4):
                    d = ro[o]
                    if act[d] and cnt[d] and rb[d]:
                        ops.append(dist.P2POp(dist.irecv, wrap(rb[d], cnt[d]), peers[d], group))
                if ops:
                    for r in dist.batch_isend_irecv(ops):
                        r.wait()
            return 0
        except Exception as e:                                   # pragma: no cover
            import sys
            print("exchange callback failed: %r" % (e,), file=sys.stderr)
            return 1

    dycore._xchg_cb = capi.EXCHANGE_FN(cb)                       # keep alive
    check(L.mw_dycore_set_exchange(dycore.h, dycore._xchg_cb, None))


def use_rccl_allreduce(coupler, dycore):
    """The column modules' sums over ranks (sponge_layer, ColumnNudger) on the dycore handle's own RCCL communicator
    (mw_dycore_rccl_allreduce_sum, ctx = the handle) instead of torch.distributed -- what a C++ host does (host/mw_facade.h)."""
    fn = C.cast(capi.lib().mw_dycore_rccl_allreduce_sum, capi.ALLREDUCE_FN)
    coupler._allreduce = (fn, dycore.h, dycore)


def _torch_allreduce(coupler, group=None):
    """-> (mw_allreduce_fn, ctx) for the sponge / nudger horizontal means: the override installed by use_rccl_allreduce, else
    torch.distributed (RCCL on GPUs); (NULL, None) on one rank."""
    ov = getattr(coupler, "_allreduce", None)
    if ov is not None:
        return ov[0], ov[1]
    import torch.distributed as dist
    if coupler.get_nranks() <= 1 or not dist.is_initialized():
        return C.cast(None, capi.ALLREDUCE_FN), None
    dev = coupler.device

    def cb(ctx, buf, n, stream):
        try:
            class _A:
                pass
            a = _A()
            a.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f8", data=(int(buf), False), version=2)
            st = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev)
            with torch.cuda.device(dev), torch.cuda.stream(st):
                t = torch.as_tensor(a, device=dev)
                if dist.get_backend(group) == "gloo":
                    h = t.cpu(); dist.all_reduce(h, group=group); t.copy_(h)
                else:
                    dist.all_reduce(t, group=group)
            return 0
        except Exception as e:                                   # pragma: no cover
            import sys
            print("allreduce callback failed: %r" % (e,), file=sys.stderr)
            return 1
    fn = capi.ALLREDUCE_FN(cb)
    coupler._allreduce_keep = fn                                 # (the callback object must outlive the call)
    return fn, None
