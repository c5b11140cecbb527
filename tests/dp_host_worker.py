"""Worker of tests/test_dp_runner_host.py: one process per rank, gloo group, everything on the CPU (no kernel is launched).

What two ranks decide when they CANNOT act: ``native_runner(..., native_data_parallel=True)`` around a pre-training TSFormer that lives
on the CPU leaves the DistributedDataParallel wrap alone on every rank, warns on rank 0 only, and the run's plumbing -- the sampler
behind the look-ahead loader, the checkpoint keys -- is what it was.  And ``TSFormer.enable_native_data_parallel`` itself on the CPU:
the state broadcast, the transport ("auto" over gloo is torch.distributed), the per-rank dropout seed streams."""
import os
import sys
import warnings

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel
from torch.utils.data import Dataset

ROOT, CKPT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
from step_amd import TSFormer                                      # noqa: E402
from step_amd.runner import LookaheadLoader, native_runner         # noqa: E402
from tests.dp_double import DistributedPretrainRunnerDouble        # noqa: E402
from tests.runner_double import masked_mae                         # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
CFG = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 1e-3, "weight_decay": 0, "eps": 1e-8, "betas": (0.9, 0.95)}},
                 "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 5.0}}}


class Origins(Dataset):
    def __len__(self):
        return 12

    def __getitem__(self, i):
        return torch.tensor(100 + i, dtype=torch.int64)


def new_model():
    torch.manual_seed(7 + rank)          # every rank initialises differently
    return TSFormer(12, 1, 96, 4, 4, 0.1, 16, 0.75, 4, 1, mode="pre-train")


# ---- the runner: no rank can act (CPU module), so nothing is unwrapped anywhere
model = new_model()
keys = list(model.state_dict())
with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    runner = native_runner(DistributedPretrainRunnerDouble, native_data_parallel=True, native_pretrain=True)(
        {"model": model, "loss": masked_mae, "scaler": (200.0, 150.0), "cl": None, "ckpt_dir": CKPT, "dataset": Origins(), "batch_size": 2})
    runner.init_training(CFG)
mine = [w for w in caught if "native_data_parallel" in str(w.message)]
assert len(mine) == (1 if rank == 0 else 0), [str(w.message) for w in caught]          # one warning, on rank 0
assert isinstance(runner.model, DistributedDataParallel) and runner.model.module is model and runner._dp_acting is False
assert type(runner.optim) is torch.optim.Adam and runner.clip_grad_param == {"max_norm": 5.0}
assert model._process_group is None and model._flat_param is None and model._seed_rank == 0
# easytorch reaches the sampler through the loader the runner wrapped
loader = runner.train_data_loader
assert isinstance(loader, LookaheadLoader)
for epoch in (1, 2):
    loader.sampler.set_epoch(epoch)
assert loader.sampler.epochs_set == [1, 2] and loader.sampler is loader.loader.sampler
got = sorted(int(v) for batch in loader.loader for v in batch)          # (the wrapped loader: origins, not staged windows)
every = [None] * world
dist.all_gather_object(every, got)
assert len(got) == 6 and sorted(sum(every, [])) == list(range(100, 112)), every          # disjoint, and together the whole dataset
# rank 0 writes the checkpoint, with the reference's keys
path = runner.save_model(1)
assert (path is not None) == (rank == 0)
dist.barrier()
assert list(torch.load(os.path.join(CKPT, "ckpt_001.pt"))["model_state_dict"]) == keys

# ---- the module's own entry point on the CPU
m = new_model()
today = TSFormer._next_seed                                   # the stream of a module without a group: the formula of a single process
base = [(torch.initial_seed() * 6364136223846793005 + c * 1442695040888963407) & ((1 << 63) - 1) for c in (1, 2, 3)]
assert [today(m) for _ in range(3)] == base
m._seed_ctr2 = 0
try:
    m.enable_native_data_parallel(collectives="rccl")
    raise AssertionError("collectives='rccl' on the CPU must raise")
except RuntimeError as ex:
    assert "GPU" in str(ex)
m.enable_native_data_parallel()
assert m._comm is None and m._seed_rank == rank
ref = [torch.empty_like(p) for p in m.parameters()]
for t, p in zip(ref, m.parameters()):
    t.copy_(p.detach())
    dist.broadcast(t, 0)
assert all(torch.equal(t, p.detach()) for t, p in zip(ref, m.parameters()))          # rank 0's values everywhere
torch.manual_seed(1234)                                        # one process-wide seed on both ranks, as a config would set it
seeds = [m._next_seed() for _ in range(3)]
want0 = [(1234 * 6364136223846793005 + c * 1442695040888963407) & ((1 << 63) - 1) for c in (1, 2, 3)]
streams = [None] * world
dist.all_gather_object(streams, seeds)
assert streams[0] == want0, (streams[0], want0)                # rank 0's stream is what it is today
assert not set(streams[0]) & set(streams[1]) and len(set(streams[1])) == 3
m.enable_native_data_parallel()                                # a second call is allowed
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
