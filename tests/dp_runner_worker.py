"""Worker of tests/test_gpu_dp_runner.py: one process per rank, gloo group, every rank on cuda:0.  ``native_runner(<double>,
native_data_parallel=True, ...)`` around easytorch's distributed protocol (tests/dp_double.py: the model arrives wrapped in
DistributedDataParallel) for the tiny pre-training TSFormer (``native_pretrain=True``) or for STEP at the size of tests/shard_worker.py
(``native_tail=True``), over the project's index-only datasets.  Two epochs of three iterations, then a second run whose rank 1 is
perturbed by one ulp before epoch 2.

STEP's gradients are not compared here: tests/shard_worker.py holds the data-parallel step to ``dp_vs_sequential < 1e-4`` on this very
problem; what this worker adds is the runner around it."""
import os
import pickle
import random
import sys

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel

ROOT, KIND, TMP = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, ROOT)
from step_amd import STEP, TSFormer                                                  # noqa: E402
from step_amd.comm import replicas_identical                                          # noqa: E402
from step_amd.optim import FusedAdamClip                                              # noqa: E402
from step_amd.runner import DeviceForecastingDataset, DevicePretrainingDataset, LookaheadLoader, native_runner      # noqa: E402
from tests import train_problem as TPb                                               # noqa: E402
from tests.dp_double import DistributedPretrainRunnerDouble, DistributedRunnerDouble  # noqa: E402
from tests.runner_double import masked_mae                                           # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
EPOCHS, ITERS, BATCH = 2, 3, 2
SAMPLES = world * ITERS * BATCH
CFG = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 2e-3, "weight_decay": 1e-5, "eps": 1e-8}},
                 "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 3.0}}}


def files(series, triples):
    d = os.path.join(TMP, f"data_rank{rank}")
    os.makedirs(d, exist_ok=True)
    paths = os.path.join(d, "data.pkl"), os.path.join(d, "index.pkl")
    with open(paths[0], "wb") as f:
        pickle.dump({"processed_data": series}, f)
    with open(paths[1], "wb") as f:
        pickle.dump({"train": triples}, f)
    return paths


if KIND == "pretrain":
    from tests.helpers import load_golden
    from tests.test_gpu_pretrain import _model
    L = 192                                               # P = 16 tokens; 9 sensors and a batch of 2: S = 18 sequences
    ORIGINS = [L + 8 + 7 * i for i in range(SAMPLES)]
    dataset = DevicePretrainingDataset(*files(TPb.make_series(9, 600), [(o - L, o, o + 12) for o in ORIGINS]), "train")

    def new_model():
        m = _model(load_golden("tsformer_pretrain_tiny"), L)
        m.train()
        m.dropout_p = 0.0
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01 * rank)                      # the ranks start apart: the wrap, and then the switch, broadcast rank 0's
        return m

    base, kwargs, loss, scaler = DistributedPretrainRunnerDouble, dict(native_pretrain=True), masked_mae, (200.0, 150.0)
else:
    from step_amd.step_loss import step_loss_native
    N, L, T_train = 48, 288, 700
    prob = TPb.Problem(N, L, T_train, n_train=32, n_eval=4)
    ORIGINS = sorted(prob.train_t[:SAMPLES])
    dataset = DeviceForecastingDataset(*files(prob.series, [(o - 12, o, o + 12) for o in ORIGINS]), "train", L)

    def new_model():
        m = TPb.build_native(N, L, T_train, prob.series, k=5, seed=rank).to(dev)
        m.train()
        m.matmul_precision = "bf16"
        return m

    base, kwargs, loss, scaler = DistributedRunnerDouble, dict(native_tail=True), step_loss_native, (prob.mean, prob.std)


def fix_masks(epoch, it):
    random.seed(1234 + 10 * epoch + it)                  # TSFormer's MaskGenerator shuffles with the random module


def new_runner(ckpt_dir):
    model = new_model()
    runner = native_runner(base, native_data_parallel=True, **kwargs)(
        {"model": model, "loss": loss, "scaler": scaler, "cl": None, "iter_per_epoch": ITERS, "ckpt_dir": ckpt_dir, "dataset": dataset,
         "batch_size": BATCH})
    assert isinstance(runner.model, DistributedDataParallel)          # what easytorch hands the runner
    runner.init_training(CFG)
    # the bare module, the fused optimizer, the switch acting
    assert runner.model is model and type(runner.model) in (STEP, TSFormer) and runner._dp_acting is True
    assert type(runner.optim) is FusedAdamClip and runner.clip_grad_param is None and model._flat_param is not None
    assert model._process_group is not None and runner.start_epoch == 0
    assert replicas_identical(model._flat_param)                      # rank 0's state everywhere, whatever the ranks started from
    return runner, model


def origins_of(batch):
    return [int(t) for t in batch[-1].t0_host]                        # the LongHistoryRef of a staged index-only batch


# ---------------------------------------------------------------------------------------------- two epochs
run1 = os.path.join(TMP, "run1")
runner, model = new_runner(run1)
assert isinstance(runner.train_data_loader, LookaheadLoader)
for epoch in range(1, EPOCHS + 1):
    seen = []
    path = runner.train_loader_epoch(epoch, fix_masks, seen)
    assert (path is not None) == (rank == 0) and len(seen) == ITERS
    mine = [o for b in seen for o in origins_of(b)]
    every = [None] * world
    dist.all_gather_object(every, mine)
    assert len(mine) == ITERS * BATCH and sorted(sum(every, [])) == ORIGINS, every          # disjoint, together the whole dataset
runner.flush_meters()
assert runner.base_calls == 0                                          # no iteration went through the double's train_iters
assert runner.train_data_loader.sampler.epochs_set == [1, 2]           # set_epoch reached the sampler through the look-ahead loader
assert runner.optim.step_count == EPOCHS * ITERS and all(m.n == EPOCHS * ITERS for m in runner.meters.values()) and runner.meters
# the gradients of the last backward: still the views of the flat buffer the backward averaged (no reducer re-homed them)
g = model._flat_grad
assert g is not None and bool(torch.isfinite(g).all())
ps = model._pt_params() if KIND == "pretrain" else model._trainable_list()
lo, hi = g.data_ptr(), g.data_ptr() + 4 * g.numel()
for q in (ps[0], ps[len(ps) // 2], ps[-1]):
    assert q.grad is None or lo <= q.grad.data_ptr() < hi
if KIND == "pretrain":
    assert all(q.grad is not None for q in (ps[0], ps[len(ps) // 2], ps[-1]))
assert replicas_identical(model._flat_param)
# the checkpoint rank 0 wrote: the reference's keys, torch Adam's format
dist.barrier()
ckpt = torch.load(os.path.join(run1, "ckpt_{:03d}.pt".format(EPOCHS)), map_location=dev)
fresh = new_model()
fresh.load_state_dict(ckpt["model_state_dict"], strict=True)
assert not any(k.startswith("module.") for k in ckpt["model_state_dict"])
for k, v in model.named_parameters():                                  # (BatchNorm's running statistics are each rank's own batches')
    assert torch.equal(v.detach(), ckpt["model_state_dict"][k]), k      # ... and it is what THIS rank trained, on every rank
adam = torch.optim.Adam(fresh.parameters(), lr=1.0)
adam.load_state_dict(ckpt["optim_state_dict"])
assert abs(adam.param_groups[0]["lr"] - 1e-3) < 1e-12 and len(adam.state) == len(ps) and all(float(s["step"]) == EPOCHS * ITERS for s in adam.state.values())
print(f"rank {rank} {KIND}: two epochs under the runner, replicas identical, checkpoint loads", flush=True)

# ---------------------------------------------------------------------------------------------- a perturbed replica is found
del runner, model, fresh, adam
runner, model = new_runner(os.path.join(TMP, "run2"))
runner.train_loader_epoch(1, fix_masks)
if rank == 1:
    flat = model._flat_param
    flat[5:6].copy_(torch.nextafter(flat[5:6], torch.full((1,), float("inf"), device=dev)))
raised = None
try:
    runner.train_loader_epoch(2, fix_masks)
except RuntimeError as ex:
    raised = str(ex)
if isinstance(model, STEP):
    model.cancel_prefetch()
everyone = [None] * world
dist.all_gather_object(everyone, raised)
assert all(m is not None and "replicas differ" in m and "epoch 2" in m for m in everyone), everyone
assert runner.optim.step_count == ITERS                                # nothing of epoch 2 ran
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
