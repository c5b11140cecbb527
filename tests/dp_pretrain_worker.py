"""Worker of tests/test_gpu_dp_pretrain.py: one process per data-parallel rank, gloo group, every rank on cuda:0, $STEP_RCCL_LIB pointing
at tests/fake_rccl for the RCCL C-API path.  The tiny pre-training TSFormer of tests/test_gpu_pretrain_tail.py (S = 18 sequences,
P = 16 tokens), dropout 0, ``random.seed`` before every forward so that the token masks are known, per-rank batches; both precisions.

  (a) after ``enable_native_data_parallel`` every rank holds rank 0's parameters, although rank 1 started from others
  (b) the flat gradient after one backward = the average of the gradients ONE process computes for both ranks' batches
  (c) after two FusedAdamClip steps ``replicas_identical`` holds; one element of rank 1 nudged by an ulp and it does not, on every rank
  (d) the same step with collectives="rccl" (through the stand-in) agrees with collectives="torch"

Tolerance of (b) and (d), relative L2 of the flat gradient.  The two sides differ only by the order of the f32 atomic additions in the
backward's column sums and split-K products; the mean itself is the same operation everywhere ((a + b) rounded once, then an exact
halving).  Measured on an MI355X on the single-process path, two backward passes over the same inputs in fresh buffers, 30 pairs per
precision, never bit-equal:  f32 3.3e-8 .. 4.65e-8,  bf16 4.2e-8 .. 5.34e-8.  Bound = 4 x the larger figure (run-to-run noise has no
fixed upper end; a handful of samples bounds it loosely) = 2.14e-7."""
import os
import random
import sys

import torch
import torch.distributed as dist

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
from step_amd.comm import replicas_identical             # noqa: E402
from step_amd.optim import FusedAdamClip                 # noqa: E402
from tests.helpers import load_golden, rel_l2            # noqa: E402
from tests.test_gpu_pretrain import _model               # noqa: E402

MEASURED_NOISE = 5.34e-8
BOUND = 4 * MEASURED_NOISE

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
g = load_golden("tsformer_pretrain_tiny")
x0 = g["in.x"].cuda()


def batch_of(r):
    return (x0 * (1.0 - 0.1 * r) + 0.05 * r).contiguous()


def new_model(precision, state=None):
    m = _model(g, x0.shape[1])
    m.train()
    m.dropout_p = 0.0
    m.matmul_precision = precision
    if state is not None:
        m.load_state_dict(state)
    return m


def backward(m, r):
    """forward + backward on rank r's batch -> the model's flat gradient buffer"""
    random.seed(100 + r)
    loss, _ = m.pretrain_tail(batch_of(r), null_val=0.0, rescale=(200.0, 150.0))
    loss.backward()
    return m._flat_grad


for precision in ("f32", "bf16"):
    # ---- (a)
    A = new_model(precision)
    with torch.no_grad():
        for p in A.parameters():
            p.add_(0.01 * rank)                          # rank 1 starts elsewhere
    A.enable_native_data_parallel(collectives="torch")
    assert A._comm is None and A._seed_rank == rank
    state = {k: v.clone() for k, v in A.state_dict().items()}
    for k, v in state.items():
        every = [torch.empty_like(v) for _ in range(world)]
        dist.all_gather(every, v)
        assert all(torch.equal(every[0], q) for q in every), f"{k} differs between the ranks after enable_native_data_parallel"
    assert torch.equal(state["output_layer.weight"].cpu(), g["param.output_layer.weight"])          # ... and they are rank 0's

    # ---- (b)
    optA = FusedAdamClip(A, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, max_norm=5.0)
    optA.zero_grad()
    fa = backward(A, rank).clone()
    C = new_model(precision, state)                      # no group: this process evaluates both ranks' batches
    acc, own = None, None
    for r in range(world):
        C.zero_grad(set_to_none=True)
        f = backward(C, r).clone()
        acc = f if acc is None else acc + f
        own = f if r == rank else own
    e_b = rel_l2(fa.cpu(), (acc / world).cpu())
    moved = rel_l2(fa.cpu(), own.cpu())                  # the other rank's gradient really arrived
    print(f"rank {rank} {precision}: data parallel vs sequential {e_b:.3e} (bound {BOUND:.3e}); vs this rank's own gradient {moved:.3e}", flush=True)
    assert moved > 1e-3, moved
    assert e_b <= BOUND, e_b
    ps = A._pt_params()
    lo, hi = A._flat_grad.data_ptr(), A._flat_grad.data_ptr() + 4 * A._flat_grad.numel()
    assert all(lo <= q.grad.data_ptr() < hi for q in (ps[0], ps[len(ps) // 2], ps[-1]))          # autograd adopted the reduced views

    # ---- (d), on the same step: a second module whose collectives are RCCL C-API calls
    R = new_model(precision, state)
    R.enable_native_data_parallel(collectives="rccl", sync_module_states=False)
    assert R._comm is not None and R._comm.world == world
    optR = FusedAdamClip(R, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, max_norm=5.0)
    optR.zero_grad()
    fr = backward(R, rank).clone()
    e_d = rel_l2(fr.cpu(), fa.cpu())
    print(f"rank {rank} {precision}: RCCL C-API path vs torch.distributed {e_d:.3e} (bound {BOUND:.3e})", flush=True)
    assert e_d <= BOUND, e_d

    # ---- (c)
    optA.step(); optR.step()
    for opt, m in ((optA, A), (optR, R)):
        opt.zero_grad()
        backward(m, rank)
        opt.step()
        assert opt.step_count == 2
        assert replicas_identical(m._flat_param) is True
    flat = A._flat_param
    at = 5                                               # (inside the first parameter, not in a padding gap)
    if rank == 1:
        flat[at:at + 1].copy_(torch.nextafter(flat[at:at + 1], torch.full((1,), float("inf"), device=flat.device)))
    assert replicas_identical(flat) is False             # on every rank, not only on the one that moved
    R._comm.close()
    R._comm = None
    # a second call replaces the transport
    A.enable_native_data_parallel(collectives="rccl")
    assert A._comm is not None and replicas_identical(A._flat_param) is True          # (the call broadcast rank 0's state again)
    A._comm.close()
    A._comm = None

dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
