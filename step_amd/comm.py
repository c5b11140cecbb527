"""Data-parallel collectives of the native training step on RCCL's C API (libstep_hip: csrc/comm.cpp, include/step_hip.h).

`NativeComm` is one RCCL communicator per process created next to a `torch.distributed` process group: rank 0 makes the 128-byte
unique id, the group's own object broadcast carries it to the other ranks (the only use of torch.distributed on this path), every
rank calls `step_comm_init_rank`.  After that the step's gradient all-reduce and the small sums of the time-sliced graph learner are
plain `ncclAllReduce` calls in stream order, issued through ctypes: no work objects, no `Work.wait()`, no stream juggling on the
host -- through `torch.distributed` the two all-reduce calls of a step cost 0.45 ms of host time in front of the optimizer even
on one rank (profiles/r04_b_C2_rccl1_noshard_timeline.md).

The reference gets its data parallelism from easytorch wrapping the model in `DistributedDataParallel` (GPU_NUM > 1:
step/STEP_PEMS04.py:30, step/STEP_PEMS07.py:29,83,117); this is the same exchange -- one mean all-reduce of the gradients per step.

Also here: ``open_transport`` (which of the two transports a module's collectives take, agreed by all ranks; shared by ``STEP`` and the
pre-training ``TSFormer``) and the replica check that stands in for DDP's guarantee of identical replicas -- ``replica_digest`` (csrc/
replica_digest.hip: 128 bits of a flat parameter buffer, read once) and ``replicas_identical`` (one 32-byte collective over them).
"""
import ctypes

import torch

from . import _lib


def available():
    """librccl can be loaded into this process (the copy torch has already loaded, when there is one)"""
    return bool(_lib.lib().step_comm_available())


def open_transport(process_group, collectives, device, min_world=1):
    """The transport of a module's data-parallel collectives, agreed by all ranks of ``process_group``: -> a ``NativeComm`` (RCCL's C
    API), or None for ``torch.distributed``.  ``collectives``: "rccl", "torch" or "auto" -- "rccl" when the group's backend is nccl
    (= RCCL) and ``device`` is a GPU, else "torch".  "auto" promises a working data-parallel step, not a particular transport: when
    librccl cannot be loaded or the communicator cannot be created on ANY rank it warns and every rank stays on torch.distributed
    (two MIN all-reduces: one before anyone enters the communicator's rendezvous, one after).  An explicit "rccl" raises instead.
    A group of ``min_world`` ranks or fewer gets no communicator (1: a single rank issues nothing; 0: it issues everything).
    Shared by ``STEP.enable_native_data_parallel`` and ``TSFormer.enable_native_data_parallel``."""
    import torch.distributed as dist
    on_gpu = device.type == "cuda"
    auto = collectives == "auto"
    if auto:
        collectives = "rccl" if (on_gpu and dist.get_backend(process_group) == "nccl") else "torch"
    if collectives not in ("rccl", "torch"):
        raise ValueError(f"collectives = {collectives!r}: expected 'auto', 'rccl' or 'torch'")
    comm = None
    if collectives == "rccl" and dist.get_world_size(process_group) > min_world:
        if not on_gpu:
            raise RuntimeError("collectives='rccl' needs the module on a GPU (move it first)")
        if not available() and not auto:
            raise RuntimeError("collectives='rccl': librccl could not be loaded into this process (STEP_RCCL_LIB names another copy)")
        usable = available()
        if auto and dist.get_world_size(process_group) > 1:
            # agree BEFORE anyone enters ncclCommInitRank: a rank whose librccl did not load would otherwise go on to the all-reduce
            # below while the others block in the communicator's rendezvous
            have = torch.tensor([1 if usable else 0], device=device, dtype=torch.int32)
            dist.all_reduce(have, op=dist.ReduceOp.MIN, group=process_group)
            usable = bool(int(have.item()))
        try:
            if not usable:
                raise RuntimeError("librccl could not be loaded on every rank")
            comm = NativeComm(process_group)
        except Exception as ex:          # noqa: BLE001
            if not auto:
                raise
            # "auto" promised a working data-parallel step, not a particular transport: say so and stay on torch.distributed
            import warnings
            warnings.warn(f"step_amd: RCCL C-API communicator could not be created ({ex}); the step's collectives stay on torch.distributed")
            comm = None
        if auto and dist.get_world_size(process_group) > 1:
            # all ranks take the same transport: one rank without a communicator puts every rank on torch.distributed
            ok = torch.tensor([1 if comm is not None else 0], device=device, dtype=torch.int32)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=process_group)
            if int(ok.item()) == 0 and comm is not None:
                comm.close()
                comm = None
    return comm


def broadcast_module_states(module, process_group):
    """what DistributedDataParallel does when it wraps a module: every rank starts from rank 0's parameters and buffers"""
    import torch.distributed as dist
    src = dist.get_global_rank(process_group, 0)
    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            d = t.detach()
            if d.is_contiguous():
                dist.broadcast(d, src, group=process_group)
            else:
                c = d.contiguous()
                dist.broadcast(c, src, group=process_group)
                d.copy_(c)


def broadcast_running_statistics(module, process_group):
    """Every rank takes rank 0's BatchNorm running statistics, in ONE broadcast of their concatenation.  Native data parallel keeps the
    parameters identical, but each rank's BatchNorm layers see that rank's batches, so the running statistics drift apart;
    ``DistributedDataParallel`` hands rank 0's buffers to every rank before each forward (``broadcast_buffers``), which is why rank 0's
    master-only evaluation and its checkpoint are THE run's.  A rank that evaluates a share of a pass needs the same statistics.  Training
    does not read them (train mode normalises with the batch's), so the parameters' trajectory is untouched.  -> floats sent"""
    import torch.distributed as dist
    bufs = [b for name, b in module.named_buffers() if name.endswith(("running_mean", "running_var")) and b.dtype == torch.float32]
    if not bufs:
        return 0
    with torch.no_grad():
        flat = torch.cat([b.detach().reshape(-1) for b in bufs])
        dist.broadcast(flat, dist.get_global_rank(process_group, 0) if process_group is not None else 0, group=process_group)
        if dist.get_rank(process_group) != 0:
            at = 0
            for b in bufs:
                b.copy_(flat[at:at + b.numel()].view_as(b))
                at += b.numel()
    return int(flat.numel())


def replica_digest(flat):
    """-> int64 ``[2]`` on ``flat``'s device: the two 64-bit words of ``step_replica_digest`` (the sum mod 2^64 and the xor of one
    splitmix64-mixed word per element and position; uint64 bit patterns, exposed as int64 since torch has no uint64 arithmetic).
    ``flat``: a contiguous f32 device tensor of fewer than 2^32 elements, at any 4-byte offset.  Nothing is read back."""
    if not (torch.is_tensor(flat) and flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous()):
        raise ValueError("replica_digest: a contiguous float32 device tensor is needed")
    out = torch.empty(2, dtype=torch.int64, device=flat.device)
    _lib.call("step_replica_digest", _lib.ptr(flat), flat.numel(), _lib.ptr(out), _lib.stream())
    return out


def replicas_identical(flat, process_group=None):
    """True when every rank of ``process_group`` holds the same bits in ``flat`` (same length on every rank): the group's MAX and MIN
    of the digest's two words from ONE 32-byte all-reduce -- the words and their complements under MAX, since max(~x) = ~min(x) in
    int64 order -- and one read-back.  Every rank sees the same four words, so every rank gets the same answer.  A collective: all
    ranks must call it."""
    import torch.distributed as dist
    d = replica_digest(flat)
    both = torch.cat([d, ~d])
    if dist.get_backend(process_group) != "nccl":
        both = both.cpu()          # (a host backend would stage the 32 bytes itself)
    dist.all_reduce(both, op=dist.ReduceOp.MAX, group=process_group)
    both = both.cpu()
    return bool(torch.equal(both[:2], ~both[2:]))


class NativeComm:
    """RCCL communicator of the current device for the ranks of `process_group` (None: the default group)."""

    def __init__(self, process_group=None):
        import torch.distributed as dist
        if not torch.cuda.is_available():
            raise RuntimeError("NativeComm needs a GPU (RCCL); CPU groups keep using torch.distributed")
        self.world = dist.get_world_size(process_group)
        self.rank = dist.get_rank(process_group)
        # every rank must leave this constructor the same way: a failure on rank 0 travels to the others as an empty id instead of
        # leaving them in the broadcast, and the finished communicator is checked with one collective of each kind before it is used
        ident, err = None, None
        if self.rank == 0:
            try:
                buf = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
                _lib.call("step_comm_unique_id", buf)
                ident = buf.raw
            except Exception as ex:          # noqa: BLE001
                err = ex
        box = [ident]
        if self.world > 1:
            src = dist.get_global_rank(process_group, 0) if process_group is not None else 0
            dist.broadcast_object_list(box, src=src, group=process_group)
        if box[0] is None:
            raise RuntimeError(f"rank 0 could not make an RCCL unique id{'' if err is None else f' ({err})'}")
        ident = ctypes.create_string_buffer(box[0], _lib.COMM_ID_BYTES)
        h = ctypes.c_void_p()
        _lib.call("step_comm_init_rank", ident, self.world, self.rank, ctypes.byref(h))
        self._h = h
        self.version = int(_lib.lib().step_comm_version())
        self._side = None
        self.self_check()

    def self_check(self):
        """one mean all-reduce (f32), one sum (f64) and one broadcast over the new communicator against their closed forms; raises on a
        wrong answer, so that a communicator that does not work is found here and not inside a backward pass"""
        w, r = self.world, self.rank
        a = torch.full((1024,), float(r + 1), device="cuda")
        b = torch.full((48,), float(r + 1), device="cuda", dtype=torch.float64)
        c = torch.full((256,), r + 7, device="cuda", dtype=torch.int64)
        self.allreduce_(a, average=True)
        self.allreduce_(b)
        self.broadcast_(c, root=0)
        torch.cuda.current_stream().synchronize()
        want_a, want_b = (w + 1) / 2.0, w * (w + 1) / 2.0
        if not (bool((a - want_a).abs().max() < 1e-5) and bool((b == want_b).all()) and bool((c == 7).all())):
            raise RuntimeError(f"RCCL communicator self-check failed on rank {r} of {w}: mean {float(a[0])} (want {want_a}), "
                               f"sum {float(b[0])} (want {want_b}), broadcast {int(c[0])} (want 7)")

    def use_side_stream(self, stream):
        """run the overlapped gradient all-reduce on `stream` (a torch.cuda.Stream the caller has checked to run concurrently with its
        compute stream, see step_arch.step._concurrent_stream); kept alive here"""
        _lib.call("step_comm_set_side_stream", self._h, ctypes.c_void_p(stream.cuda_stream))
        self._side = stream

    # ---- in stream order on the current stream
    def allreduce_(self, t, average=False):
        """t <- sum (or mean) of t over the ranks, in place, queued on the current stream"""
        code = {torch.float32: _lib.COMM_F32, torch.float64: _lib.COMM_F64, torch.uint8: _lib.COMM_U8}[t.dtype]
        _lib.call("step_comm_allreduce", self._h, _lib.ptr(t), t.numel(), code, int(average), _lib.stream())
        return t

    def broadcast_(self, t, root=0):
        v = t.view(torch.uint8) if t.dtype not in (torch.float32, torch.float64, torch.uint8) else t
        code = {torch.float32: _lib.COMM_F32, torch.float64: _lib.COMM_F64, torch.uint8: _lib.COMM_U8}[v.dtype]
        _lib.call("step_comm_broadcast", self._h, _lib.ptr(v), v.numel(), code, int(root), _lib.stream())
        return t

    # ---- the step's gradient all-reduce, overlapped with the rest of the backward
    def grad_allreduce_begin(self, chunk):
        """mean of a contiguous f32 chunk of the flat gradient buffer over the ranks, ordered behind the kernels queued so far,
        running on the communicator's own stream"""
        _lib.call("step_grad_allreduce_begin", self._h, _lib.ptr(chunk), chunk.numel(), _lib.stream())

    def grad_allreduce_join(self):
        """the current stream waits for every reduction begun since the last join"""
        _lib.call("step_grad_allreduce_join", self._h, _lib.stream())

    def close(self):
        if self._h is not None:
            _lib.lib().step_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # noqa: BLE001 -- interpreter shutdown
            pass
