"""Worker of tests/test_gpu_grad_accum_dp.py: one process per data-parallel rank, gloo group, every rank on cuda:0, $STEP_RCCL_LIB pointing
at tests/fake_rccl for the RCCL C-API path.  The tiny STEP and pre-training TSFormer of tests/test_gpu_grad_accum.py, k = 2: rank r
takes micro-batches 2 r and 2 r + 1 (noise pinned per micro-batch; pre-training dropout 0, its seeds differ per rank by design).

  (a) collectives are issued in the group's SECOND backward only (counted: torch.distributed.all_reduce / grad_allreduce_begin)
  (b) the reduced flat gradient = the mean over the ranks of each rank's sum = ONE process's float64 sum of the four single
      gradients (loss scaled by 1 / 2) divided by two, within the family's bound of tests/test_gpu_grad_accum.py
  (c) after two optimizer steps the ranks' flat parameter buffers are bit-identical (replicas_identical), on both transports"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
from step_amd.comm import replicas_identical             # noqa: E402
from step_amd.optim import FusedAdamClip                 # noqa: E402
from tests import test_gpu_grad_accum as T               # noqa: E402
from tests.helpers import load_golden, rel_l2            # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
torch.manual_seed(1234)          # the Gumbel / dropout seeds fold torch.initial_seed() in, which every process draws afresh
K = 2


def new_step():
    from tests.test_gpu_step import build_native
    m = build_native(load_golden("step_tiny"))
    m.train()
    return m


def new_pretrain():
    from tests.test_gpu_pretrain import _model
    g = load_golden("tsformer_pretrain_tiny")
    m = _model(g, g["in.x"].shape[1])
    m.train()
    return m


G_STEP = load_golden("step_tiny")
FAMILIES = {
    "step_f32": (new_step, lambda m, j: T.step_forward(m, G_STEP, j, 1.0 / K), lambda m, j: T.step_single(m, G_STEP, j, 1.0 / K), T.step_items),
    "pt_f32": (new_pretrain, lambda m, j: T.pt_forward(m, j, 0.0, 1.0 / K), lambda m, j: T.pt_single(m, j, 0.0, 1.0 / K), T.pt_items),
}

for family, (new_model, forward, single, items_of) in FAMILIES.items():
    # ---- the reference: this process alone, k = 1, all four micro-batches
    C = new_model()
    singles = [single(C, j).double().cpu() for j in range(world * K)]
    ref = sum(singles) / world
    sums = [sum(singles[K * r:K * r + K]) for r in range(world)]          # each rank's own group
    for transport in ("torch", "rccl"):
        M = new_model()
        M.enable_native_data_parallel(collectives=transport)
        assert (M._comm is not None) == (transport == "rccl")
        opt = FusedAdamClip(M, lr=1e-3, weight_decay=1e-5, max_norm=3.0)
        issued = []
        if transport == "torch":
            real = dist.all_reduce

            def counted(*a, **kw):
                issued.append("all_reduce")
                return real(*a, **kw)
            dist.all_reduce = counted
        else:
            real_begin = M._comm.grad_allreduce_begin

            def counted_begin(chunk):
                issued.append("grad_allreduce_begin")
                return real_begin(chunk)
            M._comm.grad_allreduce_begin = counted_begin
        for step in range(2):
            opt.zero_grad()
            M.set_grad_accumulation(K)
            del issued[:]
            forward(M, K * rank).backward()
            torch.cuda.synchronize()
            assert issued == [], (family, transport, issued)          # (a): nothing in the first backward
            forward(M, K * rank + 1).backward()
            torch.cuda.synchronize()
            assert len(issued) >= 1, (family, transport)          # ... everything in the second
            print(f"rank {rank} {family} {transport} step {step}: {len(issued)} collective(s), all in the second backward", flush=True)
            if step == 0:
                e = rel_l2(M._flat_grad.cpu(), ref)
                moved = rel_l2(M._flat_grad.cpu(), sums[rank])          # the other rank's micro-batches really arrived
                print(f"rank {rank} {family} {transport}: reduced gradient vs one process's mean of sums {e:.3e} (bound {T.bound(family):.3e}); "
                      f"vs this rank's own sum {moved:.3e}; vs the other rank's sum {rel_l2(M._flat_grad.cpu(), sums[1 - rank]):.3e}", flush=True)
                assert moved > 1e-3, moved
                T.held(f"rank {rank} {family} {transport}", family, M._flat_grad, ref, items_of(M))          # (b)
            opt.step()
            assert opt.step_count == step + 1
        if transport == "torch":
            dist.all_reduce = real
        assert replicas_identical(M._flat_param) is True          # (c)
        if M._comm is not None:
            M._comm.close()
            M._comm = None

dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
