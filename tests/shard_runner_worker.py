"""Worker of tests/test_gpu_shard_runner.py: one process per rank, gloo group, every rank on cuda:0.  ``native_runner(<double>,
native_data_parallel=True, shard_graph_learner=True, native_tail=True)`` around easytorch's distributed protocol with an epoch end
(tests/shard_double.py) for STEP at the size of tests/dp_runner_worker.py, but with ``T_train = 701``: ``T2 = 683`` conv2 columns, slices
of 341 and 342 -- the smallest uneven slices above the 128-column floor.  Two epochs of three iterations.

KIND ``train``: the switch acts, the training state across the ranks, rank 0's checkpoint against every rank's slices, the validation
forward between the epochs, a perturbed replica, and a rank in f32 mode that keeps every rank unsliced.  KIND ``resume`` (dropout off, fixed noise): every direction of a resume, and the
continuation against the uninterrupted run with its control.  KIND ``measure`` is no test: it prints the spread between four
uninterrupted runs, which is where CONTINUATION_BOUND comes from.

That a sliced step computes what an unsliced one does is held by tests/shard_worker.py on this problem; it is not re-proved here."""
import os
import pickle
import shutil
import sys

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel

ROOT, KIND, TMP = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, ROOT)
from step_amd import STEP                                                              # noqa: E402
from step_amd.comm import replicas_identical                                           # noqa: E402
from step_amd.optim import FusedAdamClip                                               # noqa: E402
from step_amd.runner import DeviceForecastingDataset, native_runner                    # noqa: E402
from step_amd.step_arch.discrete_graph_learning import cut_time_columns                # noqa: E402
from step_amd.step_loss import step_loss_native                                        # noqa: E402
from tests import train_problem as TPb                                                # noqa: E402
from tests.shard_double import ShardRunnerDouble                                      # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
EPOCHS, ITERS, BATCH = 2, 3, 2
SAMPLES = world * ITERS * BATCH
N, L, T_train = 48, 288, 701
T2 = T_train - 18
BOUNDS = [0, 341, 683]
A, B = BOUNDS[rank], BOUNDS[rank + 1]
CFG = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 2e-3, "weight_decay": 1e-5, "eps": 1e-8}},
                 "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 3.0}}}

# Relative L2 of the flat parameter buffer after the two epochs (six steps, the second epoch at half the rate), dropout off and the
# noise fixed, measured on an MI355X (KIND "measure": four uninterrupted sliced runs, six pairs, both ranks):
#              between uninterrupted runs       resumed vs uninterrupted     resumed WITHOUT the moments     chosen
#   prefix     7.2e-4 .. 2.03e-3 (six pairs)    2.3e-4 .. 2.8e-4 (two runs)  2.28e-2                         2^-6 = 1.56e-2
#   slice      2.0e-3 .. 8.92e-3 (six pairs)    4.9e-4 .. 1.4e-3 (two runs)  2.30e-1                         2^-4 = 6.25e-2
# chosen = 4 x (the largest value between uninterrupted runs, rounded up to a power of two), the rule of tests/test_gpu_resume.py.
# The band is wider than that file's f32-mode rows: in bf16 mode a reordered float32 atomic can move a rounded operand by 2^-9, and
# Adam turns a gradient within round-off of zero into a full +-lr, which is a fifth of a typical element of the slice (|w| <= 1/105).
# A resumed run shares its first epoch with the run it is compared to, bit for bit, which is why it lands below the band's lower end.
CONTINUATION_BOUND = {"prefix": 2.0 ** -6, "slice": 2.0 ** -4}

prob = TPb.Problem(N, L, T_train, n_train=32, n_eval=4)
ORIGINS = sorted(prob.train_t[:SAMPLES])
d = os.path.join(TMP, f"data_rank{rank}")
os.makedirs(d, exist_ok=True)
with open(os.path.join(d, "data.pkl"), "wb") as f:
    pickle.dump({"processed_data": prob.series}, f)
with open(os.path.join(d, "index.pkl"), "wb") as f:
    pickle.dump({"train": [(o - 12, o, o + 12) for o in ORIGINS]}, f)
dataset = DeviceForecastingDataset(os.path.join(d, "data.pkl"), os.path.join(d, "index.pkl"), "train", L)
FIXED = KIND != "train"                     # dropout off and one noise tensor for every forward, as tests/test_gpu_resume.py does
NOISE = torch.rand(BATCH, N * N, 2, generator=torch.Generator().manual_seed(77 + rank))


def new_model(precision="bf16"):
    m = TPb.build_native(N, L, T_train, prob.series, k=5, seed=rank).to(dev)          # the ranks start apart: rank 0's state is broadcast
    m.train()
    m.matmul_precision = precision
    if FIXED:
        m.backend.dropout = 0.0
        m.tsformer.dropout_p = 0.0
        m._noise_override = NOISE
    return m


def val_batch():
    o = torch.tensor(ORIGINS[:BATCH], dtype=torch.int64)
    return dataset.windows(o.to(dev), dev, host_origins=o)


def new_runner(ckpt_dir, shard=True, native=True, precision="bf16", acts=None):
    """a new module and a new runner around it, after ``init_training`` (which resumes from ``ckpt_dir`` if it holds a checkpoint);
    ``acts``: whether the time slices are expected to act (default: as asked for by ``shard``)"""
    model = new_model(precision)
    cls = native_runner(ShardRunnerDouble, native_data_parallel=True, native_tail=True, shard_graph_learner=shard) if native else ShardRunnerDouble
    runner = cls({"model": model, "loss": step_loss_native, "scaler": (prob.mean, prob.std), "cl": None, "iter_per_epoch": ITERS,
                  "ckpt_dir": ckpt_dir, "dataset": dataset, "batch_size": BATCH, "val_batch": val_batch()})
    assert isinstance(runner.model, DistributedDataParallel)
    runner.init_training(CFG)
    if native:
        assert runner.model is model and runner._dp_acting is True and runner._shard_acting is (shard if acts is None else acts)
        assert type(runner.optim) is FusedAdamClip and runner.clip_grad_param is None
    return runner, model


def regions(model):
    """(end of the replicated prefix, offset of the fc region, its floats) in the flat buffers"""
    lay = model._grad_layout()
    fo, fn, _ = lay["items"]["dgl.fc_w"]
    assert lay["norm_slot"] == fo - 4
    return lay["norm_slot"], fo, fn


def fc_position(runner):
    (at, (t2, a, b)), = runner.optim._sliced.items()
    assert (t2, a, b) == (T2, A, B)
    return at


def check_the_switch_acts(runner, model):
    dgl = model.discrete_graph_learning
    sh = dgl._shard
    assert sh is not None and (sh["rank"], sh["world"], sh["a"], sh["b"]) == (rank, world, A, B) and sh["bounds"] == BOUNDS
    assert runner.optim.gathered_state is True and not dgl.fc.weight.requires_grad
    ns, fo, fn = regions(model)
    assert fn == 100 * 16 * (B - A) and model._flat_param.numel() == fo + fn == runner.optim.exp_avg.numel()
    assert dgl.fc_weight_slice.data_ptr() == model._flat_param[fo:].data_ptr()
    assert replicas_identical(model._flat_param[:ns])                       # rank 0's state everywhere, whatever the ranks started from


def snapshot(runner, model):
    g = runner.optim.param_groups[0]
    return {"flat": model._flat_param.clone(), "exp_avg": runner.optim.exp_avg.clone(), "exp_avg_sq": runner.optim.exp_avg_sq.clone(),
            "step_count": runner.optim.step_count, "lr": g["lr"], "initial_lr": g["initial_lr"], "last_epoch": runner.scheduler.last_epoch}


def only_epoch(src_dir, epoch, name):
    """a checkpoint directory that holds the run's checkpoint of ``epoch`` alone (rank 0 copies, everyone waits)"""
    out = os.path.join(TMP, name)
    if rank == 0:
        os.makedirs(out)
        shutil.copy(os.path.join(src_dir, "ckpt_{:03d}.pt".format(epoch)), out)
    dist.barrier()
    return out


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def prefix_and_slice(model, flat, ref):
    ns, fo, fn = regions(model)
    return {"prefix": rel_l2(flat[:ns], ref[:ns]), "slice": rel_l2(flat[fo:fo + fn], ref[fo:fo + fn])}


def uninterrupted(name, keep_epoch_1=False):
    """two epochs in one go -> (flat parameter buffer, checkpoint directory[, snapshot after epoch 1])"""
    runner, model = new_runner(os.path.join(TMP, name))
    assert runner.start_epoch == 0
    check_the_switch_acts(runner, model)
    runner.train_loader_epoch(1)
    snap = snapshot(runner, model) if keep_epoch_1 else None
    runner.train_loader_epoch(2)
    runner.flush_meters()
    assert runner.optim.step_count == EPOCHS * ITERS
    return model._flat_param.clone(), runner.ckpt_save_dir, snap, model


# =============================================================================================== KIND "train"
def kind_train():
    run1 = os.path.join(TMP, "run1")
    runner, model = new_runner(run1)
    check_the_switch_acts(runner, model)
    dgl = model.discrete_graph_learning
    ns, fo, fn = regions(model)
    at = fc_position(runner)
    w_init = dgl.fc.weight.detach().clone()
    for epoch in range(1, EPOCHS + 1):
        seen = []
        path = runner.train_loader_epoch(epoch, None, seen)          # (a false alarm of the replica check would raise here)
        assert (path is not None) == (rank == 0) and len(seen) == ITERS
        assert runner.optim._staging is None and dgl._slice_dirty is False          # gathered, saved, released
        # validation on rank 0 between the epochs: the whole learner from the gathered matrix, no collective, no stale-slice error
        assert len(runner.validated) == (epoch if rank == 0 else 0)
        if rank == 0:
            e, pred = runner.validated[-1]
            assert e == epoch and pred.shape[:3] == (BATCH, 12, N) and bool(torch.isfinite(pred).all())
            assert model.training
    runner.flush_meters()
    assert runner.base_calls == 0
    assert runner.optim.step_count == EPOCHS * ITERS and all(m.n == EPOCHS * ITERS for m in runner.meters.values()) and runner.meters
    assert replicas_identical(model._flat_param[:ns])
    own = [None] * world
    dist.all_gather_object(own, float(model._flat_param[fo:fo + fn].double().sum()))
    assert own[0] != own[1]                                            # (the slices are not replicas: the whole buffer would not pass)
    # the checkpoint rank 0 wrote: the reference's keys, torch Adam's format, every rank's slice in its columns
    dist.barrier()
    ckpt = torch.load(os.path.join(run1, "ckpt_{:03d}.pt".format(EPOCHS)), map_location=dev)
    fresh = TPb.build_native(N, L, T_train, prob.series, k=5, seed=5).to(dev)
    assert list(ckpt["model_state_dict"]) == list(fresh.state_dict()) and not any("fc_weight_slice" in k for k in ckpt["model_state_dict"])
    fresh.load_state_dict(ckpt["model_state_dict"], strict=True)
    file_w = ckpt["model_state_dict"]["discrete_graph_learning.fc.weight"]
    assert file_w.shape == (100, 16 * T2)
    assert torch.equal(cut_time_columns(file_w, T2, A, B), dgl.fc_weight_slice.detach())
    assert not torch.equal(file_w, w_init)                             # the control: the gather ran
    assert not torch.equal(cut_time_columns(file_w, T2, A, B), cut_time_columns(w_init, T2, A, B))
    assert not torch.equal(cut_time_columns(file_w, T2, *BOUNDS[1 - rank:3 - rank]), cut_time_columns(w_init, T2, *BOUNDS[1 - rank:3 - rank]))
    state = ckpt["optim_state_dict"]["state"]
    for key, buf in (("exp_avg", runner.optim.exp_avg), ("exp_avg_sq", runner.optim.exp_avg_sq)):
        assert state[at][key].shape == (100, 16 * T2)
        assert torch.equal(cut_time_columns(state[at][key], T2, A, B), buf[fo:fo + fn].view(100, -1)), key
        assert float(state[at][key].abs().max()) > 0
    for k, v in model.named_parameters():                              # every replicated parameter, and the gathered fc.weight
        if not k.endswith("fc_weight_slice"):
            assert torch.equal(v.detach(), ckpt["model_state_dict"][k]), k
    params = list(fresh.parameters())
    assert params[at] is fresh.discrete_graph_learning.fc.weight
    adam = torch.optim.Adam(params, lr=1.0)
    adam.load_state_dict(ckpt["optim_state_dict"])
    assert abs(adam.param_groups[0]["lr"] - 1e-3) < 1e-12 and len(adam.state) == len(model._trainable_list())
    assert all(float(s["step"]) == EPOCHS * ITERS for s in adam.state.values())
    assert adam.state[params[at]]["exp_avg"].shape == (100, 16 * T2)
    print(f"rank {rank}: two epochs in time slices, {len(ckpt['model_state_dict'])} keys, slices and moments in their columns", flush=True)

    # ------------------------------------------------------------------------------------------ a perturbed replica is still found
    del runner, model, fresh, adam, ckpt
    runner, model = new_runner(os.path.join(TMP, "run2"))
    runner.train_loader_epoch(1)
    if rank == 1:
        flat = model._flat_param
        flat[5:6].copy_(torch.nextafter(flat[5:6], torch.full((1,), float("inf"), device=dev)))
    raised = None
    try:
        runner.train_loader_epoch(2)
    except RuntimeError as ex:
        raised = str(ex)
    model.cancel_prefetch()
    everyone = [None] * world
    dist.all_gather_object(everyone, raised)
    assert all(m is not None and "replicas differ" in m and "epoch 2" in m for m in everyone), everyone
    assert runner.optim.step_count == ITERS                            # nothing of epoch 2 ran

    # ------------------------------------------------------------------------------------------ one rank that cannot slice: nobody does
    import warnings
    del runner, model
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        runner, model = new_runner(os.path.join(TMP, "run3"), precision="f32" if rank == 1 else "bf16", acts=False)
    mine = [w for w in caught if "shard_graph_learner needs" in str(w.message)]
    assert len(mine) == (1 if rank == 0 else 0), [str(w.message) for w in caught]          # one warning, on rank 0
    assert model.discrete_graph_learning._shard is None and runner.optim._sliced is None and model._process_group is not None
    assert model.discrete_graph_learning.fc.weight.requires_grad and replicas_identical(model._flat_param)


# =============================================================================================== KIND "resume"
def check_restored_in_slices(runner, model, snap):
    """directly after init_training: everything is the bits of the moment the checkpoint was written"""
    assert runner.start_epoch == 1 and runner.resume_errors == []
    ns, fo, fn = regions(model)
    flat, opt = model._flat_param, runner.optim
    assert torch.equal(flat[:ns], snap["flat"][:ns])                   # the replicated prefix
    assert torch.equal(flat[fo:fo + fn], snap["flat"][fo:fo + fn])     # this rank's slice
    assert torch.equal(opt.exp_avg, snap["exp_avg"]) and torch.equal(opt.exp_avg_sq, snap["exp_avg_sq"])
    assert float(opt.exp_avg[fo:fo + fn].abs().max()) > 0
    g = opt.param_groups[0]
    assert opt.step_count == snap["step_count"] == ITERS
    assert g["lr"] == snap["lr"] and abs(g["lr"] - 1e-3) < 1e-12 and g["initial_lr"] == snap["initial_lr"] == 2e-3
    assert runner.scheduler.optimizer is opt and runner.scheduler.last_epoch == snap["last_epoch"] == 1
    assert replicas_identical(flat[:ns])


def continued(src_dir, name, carry_moments=True, snap=None):
    runner, model = new_runner(only_epoch(src_dir, 1, name))
    check_the_switch_acts(runner, model)
    if snap is not None:
        check_restored_in_slices(runner, model, snap)
    if not carry_moments:
        runner.optim.exp_avg.zero_()
        runner.optim.exp_avg_sq.zero_()
        runner.optim.step_count = 0
    runner.train_loader_epoch(2)
    runner.flush_meters()
    return model._flat_param.clone()


def kind_resume():
    full, run, snap, model = uninterrupted("full", keep_epoch_1=True)
    again, _, _, _ = uninterrupted("again")
    # sliced -> sliced
    resumed = continued(run, "resumed", snap=snap)
    control = continued(run, "control", carry_moments=False)
    noise, err, without = (prefix_and_slice(model, x, full) for x in (again, resumed, control))
    print(f"rank {rank} continuation: between two uninterrupted runs {noise}, resumed {err}, resumed without the moments {without}, "
          f"bound {CONTINUATION_BOUND}", flush=True)
    every_direction(run, snap)
    for part, bound in CONTINUATION_BOUND.items():
        assert noise[part] <= bound, (part, noise)          # the bound is the noise's, not the resume's
        assert err[part] <= bound, (part, err)
        assert without[part] > bound, (part, without)          # the control: a resume that lost the moments is told apart


def every_direction(run, snap):
    ckpt = torch.load(os.path.join(run, "ckpt_001.pt"), map_location=dev)
    state = ckpt["optim_state_dict"]["state"]

    # sliced -> unsliced, under the native runner: the whole matrix and its whole moments, and the run goes on
    runner, whole = new_runner(only_epoch(run, 1, "to_unsliced"), shard=False)
    assert whole.discrete_graph_learning._shard is None and runner.start_epoch == 1 and runner.optim.step_count == ITERS
    assert runner.optim._sliced is None
    lay = whole._grad_layout()
    fo, fn, _ = lay["items"]["dgl.fc_w"]
    assert fn == 100 * 16 * T2
    at = next(i for i, v in runner.optim._index.items() if v[0] == "dgl.fc_w")
    assert torch.equal(whole.discrete_graph_learning.fc.weight.detach(), ckpt["model_state_dict"]["discrete_graph_learning.fc.weight"])
    assert torch.equal(runner.optim.exp_avg[fo:fo + fn].view(100, -1), state[at]["exp_avg"])
    assert torch.equal(runner.optim.exp_avg_sq[fo:fo + fn].view(100, -1), state[at]["exp_avg_sq"])
    assert torch.equal(cut_time_columns(whole.discrete_graph_learning.fc.weight.detach(), T2, A, B), snap["flat"][-100 * 16 * (B - A):].view(100, -1))
    runner.train_loader_epoch(2)
    runner.flush_meters()
    assert runner.optim.step_count == EPOCHS * ITERS and replicas_identical(whole._flat_param)
    unsliced_dir = runner.ckpt_save_dir
    del runner, whole

    # sliced -> the reference's runner (the double itself: torch's Adam around the DistributedDataParallel wrap)
    runner, wrapped = new_runner(only_epoch(run, 1, "to_reference"), native=False)
    assert type(runner.optim) is torch.optim.Adam and isinstance(runner.model, DistributedDataParallel)
    assert runner.resume_errors == [] and runner.start_epoch == 1 and runner.scheduler.last_epoch == 1
    params = runner.optim.param_groups[0]["params"]
    assert params[at] is wrapped.discrete_graph_learning.fc.weight and len(runner.optim.state) == len(state)
    for i, st in state.items():
        got = runner.optim.state[params[i]]
        assert float(got["step"]) == ITERS and torch.equal(got["exp_avg"], st["exp_avg"]) and torch.equal(got["exp_avg_sq"], st["exp_avg_sq"]), i
    assert torch.equal(params[at].detach(), ckpt["model_state_dict"]["discrete_graph_learning.fc.weight"])
    del runner, wrapped, params

    # unsliced -> sliced: the checkpoint the unsliced run above wrote after ITS epoch 2 (torch's format around the whole matrix)
    ckpt = torch.load(os.path.join(unsliced_dir, "ckpt_002.pt"), map_location=dev)
    state = ckpt["optim_state_dict"]["state"]
    runner, model = new_runner(only_epoch(unsliced_dir, 2, "to_sliced"))
    check_the_switch_acts(runner, model)
    assert runner.start_epoch == 2 and runner.resume_errors == [] and runner.optim.step_count == EPOCHS * ITERS
    ns, fo, fn = regions(model)
    assert fc_position(runner) == at
    file_w = ckpt["model_state_dict"]["discrete_graph_learning.fc.weight"]
    assert torch.equal(model.discrete_graph_learning.fc_weight_slice.detach(), cut_time_columns(file_w, T2, A, B))
    for key, buf in (("exp_avg", runner.optim.exp_avg), ("exp_avg_sq", runner.optim.exp_avg_sq)):
        assert torch.equal(buf[fo:fo + fn].view(100, -1), cut_time_columns(state[at][key], T2, A, B)), key
        assert float(buf[fo:fo + fn].abs().max()) > 0
    for i, (name, off, p) in runner.optim._index.items():
        if i != at:
            assert torch.equal(runner.optim.exp_avg[off:off + p.numel()].view(p.shape), state[i]["exp_avg"]), name
    runner.train_loader_epoch(3)          # and the run goes on in slices, the replica check included
    runner.flush_meters()
    assert runner.optim.step_count == (EPOCHS + 1) * ITERS and replicas_identical(model._flat_param[:ns])


# =============================================================================================== KIND "measure" (no test)
def kind_measure():
    runs = []
    for i in range(4):
        flat, _, _, model = uninterrupted(f"m{i}")
        runs.append(flat)
    pairs = [prefix_and_slice(model, runs[i], runs[j]) for i in range(4) for j in range(i)]
    for part in ("prefix", "slice"):
        vals = sorted(p[part] for p in pairs)
        print(f"rank {rank} measure {part}: six pairs {vals[0]:.3e} .. {vals[-1]:.3e}  {['%.3e' % v for v in vals]}", flush=True)


{"train": kind_train, "resume": kind_resume, "measure": kind_measure}[KIND]()
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
