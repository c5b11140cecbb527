"""Checkpoint resume on the device: FusedAdamClip's state in torch.optim.Adam's format against a live torch Adam (both ways), and a run
resumed through ``native_runner`` around easytorch's checkpoint protocol (tests/resume_double.py) in every direction -- written by the
fused optimizer or by torch's, resumed under either -- for STEP (the step_tiny golden's module, set up as in
tests/test_gpu_step.py::test_fused_adam_clip_matches_torch) and for TSFormer pre-training (``native_pretrain=True``, the
tsformer_pretrain_tiny module of tests/test_gpu_pretrain_tail.py).  Dropout is off and the noise fixed (the Gumbel noise of the golden;
``random.seed`` per iteration for the masks), so that a run differs from its repetition only by what float32 atomics reorder.

A saved run is two epochs of two iterations under ``MultiStepLR(milestones=[1])`` with easytorch's ``save_model(epoch)`` after each
epoch.  The resume tests read the checkpoint of epoch 1 (two steps taken, the rate already decayed: lr != initial_lr), the continuation
test the one of epoch 2.  Host side of the format: tests/test_optim_state_host.py."""
import copy
import functools
import os
import random
import shutil

import pytest
import torch

from tests.helpers import load_golden, max_abs
from tests.resume_double import ResumeProtocol, ResumeRunnerDouble
from tests.runner_double import masked_mae
from tests.test_gpu_pretrain_tail import PretrainRunnerDouble

pytestmark = pytest.mark.gpu

CFG = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 2e-3, "weight_decay": 1e-5, "eps": 1e-8}},
                 "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 3.0}}}
KINDS = ("step", "pretrain")


class ResumePretrainRunnerDouble(ResumeProtocol, PretrainRunnerDouble):
    """PretrainRunnerDouble (the TSFormer runner's forward) with the checkpoint protocol"""


# ---------------------------------------------------------------------------------------------- the two problems
def new_model(kind):
    if kind == "step":
        from tests.test_gpu_step import build_native
        g = load_golden("step_tiny")
        torch.manual_seed(0)
        model = build_native(g)
        model.train()
        model.backend.dropout = 0.0
        model.tsformer.dropout_p = 0.0
        model._noise_override = g["in.u"]
        return model
    from tests.test_gpu_pretrain import _model
    g = load_golden("tsformer_pretrain_tiny")
    model = _model(g, g["in.x"].shape[1])
    model.train()
    model.dropout_p = 0.0
    return model


@functools.lru_cache(maxsize=None)
def batches(kind):
    """two batches an epoch"""
    if kind == "step":
        from tests.test_gpu_step import inputs_of
        hist, long_hist, fut = inputs_of(load_golden("step_tiny"))
        return [(fut, hist, long_hist), (fut.flip(0).contiguous(), hist.flip(0).contiguous(), long_hist.flip(0).contiguous())]
    from tests.test_gpu_pretrain_tail import runner_problem
    return runner_problem()[1]


def fix_masks(epoch, it):
    random.seed(1234 + 10 * epoch + it)          # TSFormer's MaskGenerator shuffles with the random module


def new_runner(kind, native, all_params, ckpt_dir):
    """a new module and a new runner around it, after ``init_training`` (which resumes from ``ckpt_dir`` if it holds a checkpoint)"""
    from step_amd.runner import native_runner
    from step_amd.step_loss import step_loss_native
    base = ResumeRunnerDouble if kind == "step" else ResumePretrainRunnerDouble
    cls = native_runner(base, native_pretrain=kind == "pretrain") if native else base
    if kind == "step":
        mean, std = [float(x) for x in load_golden("step_tiny")["meta.scaler"]]
        loss = step_loss_native
    else:
        (mean, std), loss = (200.0, 150.0), masked_mae
    runner = cls({"model": new_model(kind), "loss": loss, "scaler": (mean, std), "cl": None, "iter_per_epoch": 2,
                  "ckpt_dir": ckpt_dir, "all_params": all_params})
    runner.init_training(CFG)
    return runner


def train(runner, kind, epochs):
    """easytorch's loop from the runner's ``start_epoch`` on, a checkpoint after every epoch"""
    for epoch in range(runner.start_epoch + 1, epochs + 1):
        runner.train_epoch(epoch, batches(kind), fix_masks)
    if hasattr(runner, "flush_meters"):
        runner.flush_meters()


def snapshot(runner):
    """what a checkpoint of this moment has to bring back (clones)"""
    from step_amd.optim import FusedAdamClip
    opt = runner.optim
    snap = {"model": {k: v.clone() for k, v in runner.model.state_dict().items()},
            "state": copy.deepcopy(opt.state_dict()["state"]), "lr": opt.param_groups[0]["lr"],
            "initial_lr": opt.param_groups[0]["initial_lr"], "scheduler": copy.deepcopy(runner.scheduler.state_dict())}
    if isinstance(opt, FusedAdamClip):
        snap.update(exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), step_count=opt.step_count)
    return snap


_SAVED = {}


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """saved(kind, native, all_params) -> {"dir", 1: snapshot after epoch 1, 2: after epoch 2}, each run once"""
    def get(kind, native, all_params):
        key = (kind, native, all_params)
        if key not in _SAVED:
            d = str(tmp_path_factory.mktemp("run_{}_{}_{}".format(kind, "native" if native else "torch", "all" if all_params else "trainable")))
            runner = new_runner(kind, native, all_params, d)
            assert runner.start_epoch == 0 and len(runner.resume_errors) == 1          # nothing to resume from
            out = {"dir": d}
            for epoch in (1, 2):
                train(runner, kind, epoch)
                out[epoch] = snapshot(runner)
                runner.start_epoch = epoch
            _SAVED[key] = out
        return _SAVED[key]
    return get


def only_epoch(run, epoch, tmp_path):
    """a checkpoint directory that holds the run's checkpoint of ``epoch`` alone"""
    d = str(tmp_path / "resume")
    os.makedirs(d)
    shutil.copy(os.path.join(run["dir"], "ckpt_{:03d}.pt".format(epoch)), d)
    return d


def flat_gaps(model, buf):
    """the floats of a flat buffer that belong to no parameter"""
    from step_amd.optim import flat_items
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for _, off, p in flat_items(model):
        keep[off:off + p.numel()] = False
    return buf[keep]


def check_model_restored(runner, snap):
    sd = runner.model.state_dict()
    assert list(sd) == list(snap["model"])
    for k, v in snap["model"].items():          # every parameter and every BatchNorm buffer
        assert torch.equal(sd[k], v), k


def check_schedule_restored(runner, snap, epoch):
    g = runner.optim.param_groups[0]
    assert g["lr"] == snap["lr"] and g["initial_lr"] == snap["initial_lr"] == CFG["TRAIN"]["OPTIM"]["PARAM"]["lr"]
    assert g["lr"] == pytest.approx(1e-3)          # decayed at milestone 1: not the base rate
    assert runner.scheduler.optimizer is runner.optim and runner.scheduler.last_epoch == epoch
    assert runner.scheduler.base_lrs == [snap["initial_lr"]]
    assert runner.scheduler.state_dict() == runner.scheduler_after_resume          # what the protocol left on the replaced scheduler
    assert runner.scheduler_after_resume["last_epoch"] == epoch


# ---------------------------------------------------------------------------------------------- optimizer level (tests 1 and 2)
def shadowed_steps(n):
    """n fused steps on the STEP module beside a shadow torch Adam + clip_grad_norm_ fed the same gradients
    (tests/test_gpu_step.py::test_fused_adam_clip_matches_torch) -> model, fused, shadow parameters, torch Adam, one_step(optimizers)"""
    from oracle import step_oracle as O
    from step_amd.optim import FusedAdamClip
    from tests.test_gpu_step import inputs_of
    g = load_golden("step_tiny")
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs_of(g)
    model = new_model("step")
    named = [(n_, p) for n_, p in model.named_parameters() if p.requires_grad]
    shadow = [p.detach().clone().requires_grad_(True) for _, p in named]
    hyper = dict(lr=2e-3, weight_decay=1e-5, eps=1e-8)
    fused = FusedAdamClip(model, max_norm=3.0, params=[p for _, p in named], **hyper)          # positions as in the shadow list
    topt = torch.optim.Adam(shadow, **hyper)
    lay = model._grad_layout()
    assert any(n_ % 4 for _, n_, _ in lay["items"].values()) and lay["norm_slot"] is not None          # padding and the spare slot are there
    count = [0]

    def one_step(f, t):
        f.zero_grad(set_to_none=True)
        t.zero_grad(set_to_none=True)
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=count[0], epoch=1)
        O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef).backward()
        for sp, (_, p) in zip(shadow, named):
            sp.grad = None if p.grad is None else p.grad.detach().clone()
        torch.nn.utils.clip_grad_norm_([sp for sp in shadow if sp.grad is not None], max_norm=3.0)
        t.step()
        f.step()
        count[0] += 1

    for _ in range(n):
        one_step(fused, topt)
    return model, named, fused, shadow, topt, hyper, one_step


def check_within_the_fused_versus_torch_bound(named, shadow):
    worst = 0.0
    for sp, (n, p) in zip(shadow, named):
        err, bound = max_abs(p.detach().cpu(), sp.detach().cpu()), 2e-6 + 2e-5 * float(sp.detach().abs().max())
        worst = max(worst, err / bound)
        assert err < bound, (n, err, bound)
    print("worst error / bound", worst)


def test_fused_state_loads_into_torch_adam_and_the_fourth_steps_agree():
    model, named, fused, shadow, topt, hyper, one_step = shadowed_steps(3)
    sd = fused.state_dict()
    fresh = torch.optim.Adam(shadow, lr=1.0)          # everything but the parameters comes from the loaded state
    fresh.load_state_dict(copy.deepcopy(sd))
    assert fresh.param_groups[0]["lr"] == 2e-3 and fresh.param_groups[0]["weight_decay"] == 1e-5
    with_state = 0
    for i, (sp, (n, p)) in enumerate(zip(shadow, named)):
        assert (sp in fresh.state) == (i in sd["state"]) == (sp in topt.state), n
        if i in sd["state"]:
            with_state += 1
            st = fresh.state[sp]
            assert float(st["step"]) == 3.0 and st["exp_avg"].shape == p.shape
            assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
            lo = fused.exp_avg.data_ptr()
            assert lo <= sd["state"][i]["exp_avg"].data_ptr() < lo + 4 * fused.exp_avg.numel(), n          # a view of the flat buffer
    assert with_state == len(model._trainable_list())
    one_step(fused, fresh)
    assert fused.step_count == 4 and all(float(st["step"]) == 4.0 for st in fresh.state.values())
    check_within_the_fused_versus_torch_bound(named, shadow)


def test_torch_state_loads_into_a_fresh_fused_optimizer_and_the_fourth_steps_agree():
    from step_amd.optim import FusedAdamClip
    model, named, fused, shadow, topt, hyper, one_step = shadowed_steps(3)
    del fused
    fresh = FusedAdamClip(model, lr=1.0, max_norm=3.0, params=[p for _, p in named])
    assert fresh.step_count == 0 and not fresh.exp_avg.any()
    fresh.exp_avg.fill_(float("nan"))          # whatever was in the gaps must not survive
    fresh.exp_avg_sq.fill_(float("nan"))
    tsd = topt.state_dict()
    fresh.load_state_dict(tsd)
    assert fresh.step_count == 3 and fresh.param_groups[0]["lr"] == 2e-3 and fresh.param_groups[0]["weight_decay"] == 1e-5
    gaps = flat_gaps(model, fresh.exp_avg)
    assert gaps.numel() >= 4 and not gaps.any() and not flat_gaps(model, fresh.exp_avg_sq).any()
    mine = fresh.state_dict()["state"]
    assert sorted(mine) == sorted(tsd["state"]) and len(mine) == len(model._trainable_list())
    for i, st in tsd["state"].items():
        assert torch.equal(mine[i]["exp_avg"], st["exp_avg"]) and torch.equal(mine[i]["exp_avg_sq"], st["exp_avg_sq"]), named[i][0]
    one_step(fresh, topt)
    assert fresh.step_count == 4
    check_within_the_fused_versus_torch_bound(named, shadow)


# ---------------------------------------------------------------------------------------------- through the runner (tests 3, 4 and 5)
@pytest.mark.parametrize("all_params", (True, False), ids=("all_parameters", "trainable_only"))
@pytest.mark.parametrize("kind", KINDS)
def test_native_checkpoint_resumes_under_the_native_runner(kind, all_params, saved, tmp_path):
    from step_amd.optim import FusedAdamClip
    run = saved(kind, True, all_params)
    snap = run[1]
    assert snap["step_count"] == 2 and float(snap["exp_avg"].abs().max()) > 0
    runner = new_runner(kind, True, all_params, only_epoch(run, 1, tmp_path))
    opt = runner.optim
    assert isinstance(opt, FusedAdamClip) and runner.clip_grad_param is None and runner.resume_errors == []
    assert runner.start_epoch == 1 and opt.step_count == 2
    assert torch.equal(opt.exp_avg, snap["exp_avg"]) and torch.equal(opt.exp_avg_sq, snap["exp_avg_sq"])
    check_schedule_restored(runner, snap, 1)
    check_model_restored(runner, snap)
    train(runner, kind, 2)          # and the resumed run goes on
    assert opt.step_count == 4 and all(torch.isfinite(v).all() for v in runner.model.state_dict().values())


@pytest.mark.parametrize("all_params", (True, False), ids=("all_parameters", "trainable_only"))
@pytest.mark.parametrize("kind", KINDS)
def test_torch_checkpoint_resumes_under_the_native_runner(kind, all_params, saved, tmp_path):
    from step_amd.optim import FusedAdamClip
    run = saved(kind, False, all_params)
    snap = run[1]
    runner = new_runner(kind, True, all_params, only_epoch(run, 1, tmp_path))
    opt = runner.optim
    assert isinstance(opt, FusedAdamClip) and runner.resume_errors == [] and runner.start_epoch == 1 and opt.step_count == 2
    mine = opt.state_dict()["state"]
    flat = runner.model._pt_params() if kind == "pretrain" else runner.model._trainable_list()
    assert sorted(mine) == sorted(snap["state"]) and len(mine) == len(flat)
    for i, st in snap["state"].items():
        assert float(st["step"]) == 2.0
        assert torch.equal(mine[i]["exp_avg"], st["exp_avg"]) and torch.equal(mine[i]["exp_avg_sq"], st["exp_avg_sq"]), i
    assert not flat_gaps(runner.model, opt.exp_avg).any() and not flat_gaps(runner.model, opt.exp_avg_sq).any()
    check_schedule_restored(runner, snap, 1)
    check_model_restored(runner, snap)
    train(runner, kind, 2)
    assert opt.step_count == 4 and all(torch.isfinite(v).all() for v in runner.model.state_dict().values())


@pytest.mark.parametrize("all_params", (True, False), ids=("all_parameters", "trainable_only"))
@pytest.mark.parametrize("kind", KINDS)
def test_native_checkpoint_resumes_under_the_reference_protocol(kind, all_params, saved, tmp_path):
    run = saved(kind, True, all_params)
    snap = run[1]
    runner = new_runner(kind, False, all_params, only_epoch(run, 1, tmp_path))
    assert type(runner.optim) is torch.optim.Adam
    assert runner.resume_errors == []          # (a KeyError on the optimizer state is swallowed by the protocol)
    assert runner.start_epoch == 1 and runner.scheduler.last_epoch == 1
    params = runner.optim.param_groups[0]["params"]
    assert len(snap["state"]) > 0 and len(runner.optim.state) == len(snap["state"])
    for i, st in snap["state"].items():
        got = runner.optim.state[params[i]]
        assert float(got["step"]) == 2.0 and got["exp_avg"].shape == params[i].shape
        assert torch.equal(got["exp_avg"], st["exp_avg"]) and torch.equal(got["exp_avg_sq"], st["exp_avg_sq"]), i
    g = runner.optim.param_groups[0]
    assert g["lr"] == snap["lr"] and g["initial_lr"] == snap["initial_lr"]
    check_model_restored(runner, snap)
    train(runner, kind, 2)
    assert all(float(st["step"]) == 4.0 for st in runner.optim.state.values())
    assert all(torch.isfinite(v).all() for v in runner.model.state_dict().values())


# ---------------------------------------------------------------------------------------------- continuation (test 6)
def rel_l2_flat(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def uninterrupted(kind, ckpt_dir, epochs=3):
    """-> the flat parameter buffer after ``epochs`` epochs in one go"""
    runner = new_runner(kind, True, True, ckpt_dir)
    assert runner.start_epoch == 0
    train(runner, kind, epochs)
    assert runner.optim.step_count == 2 * epochs
    return runner.model._flat_param.clone()


def continued(kind, run, ckpt_dir, carry_moments=True, epochs=3):
    """-> the flat parameter buffer of a run resumed from the saved run's newest checkpoint (epoch 2) and trained up to ``epochs``;
    ``carry_moments=False``: with the optimizer state a resume had before (zero moments, step count 0)"""
    shutil.copytree(run["dir"], ckpt_dir)
    runner = new_runner(kind, True, True, ckpt_dir)
    assert runner.start_epoch == 2 and runner.optim.step_count == 4
    assert torch.equal(runner.optim.exp_avg, run[2]["exp_avg"]) and runner.optim.param_groups[0]["lr"] == run[2]["lr"]
    if not carry_moments:
        runner.optim.exp_avg.zero_()
        runner.optim.exp_avg_sq.zero_()
        runner.optim.step_count = 0
    train(runner, kind, epochs)
    return runner.model._flat_param.clone()


# relative L2 of the flat parameter buffers after three epochs (six steps), measured on an MI355X with four uninterrupted runs and
# two resumed ones of each problem:
#              between uninterrupted runs       resumed vs uninterrupted     resumed WITHOUT the moments    chosen
#   step       7.3e-6 .. 8.62e-5 (six pairs)    7.5e-6 .. 8.63e-5            1.38e-2                        2^-11 = 4.9e-4
#   pretrain   6.3e-7 .. 1.86e-6 (six pairs)    8.8e-7 .. 2.42e-6            1.54e-2                        2^-17 = 7.6e-6
# chosen = 4 x (the largest value between uninterrupted runs, rounded up to a power of two): what float32 atomics reorder, amplified
# by Adam (a gradient within round-off of zero moves its parameter by a full +-lr).  The run moves the parameters by 5e-2.
CONTINUATION_BOUND = {"step": 2.0 ** -11, "pretrain": 2.0 ** -17}


@pytest.mark.parametrize("kind", KINDS)
def test_a_resumed_run_continues_like_the_uninterrupted_one(kind, saved, tmp_path):
    run = saved(kind, True, True)
    full = uninterrupted(kind, str(tmp_path / "full"))
    again = uninterrupted(kind, str(tmp_path / "again"))
    resumed = continued(kind, run, str(tmp_path / "resumed"))
    control = continued(kind, run, str(tmp_path / "control"), carry_moments=False)
    noise, err, without = rel_l2_flat(again, full), rel_l2_flat(resumed, full), rel_l2_flat(control, full)
    bound = CONTINUATION_BOUND[kind]
    print(kind, "between two uninterrupted runs", noise, "resumed", err, "resumed without the moments", without, "bound", bound)
    assert noise <= bound          # the bound is the noise's, not the resume's
    assert err <= bound
    assert without > bound          # the control: this problem tells a resume that lost the moments from one that kept them
