"""``native_runner(..., native_data_parallel=True, shard_graph_learner=True)`` with two ranks on one device around easytorch's
distributed protocol with an epoch end (tests/shard_double.py, tests/shard_runner_worker.py): every rank trains one time slice of the
graph learner, the replica check covers the replicated prefix, the epoch's end gathers ``fc.weight`` and its moments so that rank 0
validates the whole learner and writes the reference's checkpoint -- which resumes sliced, unsliced, under the reference's protocol and
in a single process.  Host side of the format: tests/test_shard_state_host.py."""
import inspect
import os

import pytest
import torch

from tests.two_ranks import run_two_ranks

pytestmark = pytest.mark.gpu


def test_the_switch_is_an_argument_of_native_runner():
    from step_amd.runner import native_runner
    from tests.runner_double import RunnerDouble
    assert inspect.signature(native_runner).parameters["shard_graph_learner"].default is False
    native_runner(RunnerDouble, native_data_parallel=True, shard_graph_learner=True)          # (a TypeError before the switch existed)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """the ``train`` worker, once: -> the directory that holds its runs (``run1``: two epochs in time slices)"""
    tmp = tmp_path_factory.mktemp("shard_runner")
    run_two_ranks("shard_runner_worker.py", "train", tmp, timeout=300)
    return str(tmp)


def test_two_ranks_train_in_time_slices_and_rank_0_writes_the_whole_checkpoint(trained):
    assert os.path.isfile(os.path.join(trained, "run1", "ckpt_002.pt"))


def test_a_sliced_checkpoint_resumes_in_a_single_process(trained, tmp_path):
    """no process group: the native runner around easytorch's checkpoint protocol, the whole graph learner, one optimizer"""
    import shutil
    from step_amd.optim import FusedAdamClip
    from step_amd.runner import native_runner
    from step_amd.step_loss import step_loss_native
    from tests import train_problem as TPb
    from tests.resume_double import ResumeRunnerDouble
    N, L, T_train, T2 = 48, 288, 701, 683
    cfg = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 2e-3, "weight_decay": 1e-5, "eps": 1e-8}},
                     "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 3.0}}}
    shutil.copy(os.path.join(trained, "run1", "ckpt_001.pt"), tmp_path)
    dev = torch.device("cuda:0")
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt_001.pt"), map_location=dev)
    prob = TPb.Problem(N, L, T_train, n_train=32, n_eval=4)
    model = TPb.build_native(N, L, T_train, prob.series, k=5, seed=9).to(dev)
    model.train()
    model.matmul_precision = "bf16"
    runner = native_runner(ResumeRunnerDouble, native_data_parallel=True, shard_graph_learner=True, native_tail=True)(
        {"model": model, "loss": step_loss_native, "scaler": (prob.mean, prob.std), "cl": None, "iter_per_epoch": 3, "ckpt_dir": str(tmp_path)})
    runner.init_training(cfg)
    opt = runner.optim
    assert runner._dp_acting is False and runner._shard_acting is False and model.discrete_graph_learning._shard is None
    assert isinstance(opt, FusedAdamClip) and opt._sliced is None and runner.resume_errors == []
    assert runner.start_epoch == 1 and opt.step_count == 3 and abs(opt.param_groups[0]["lr"] - 1e-3) < 1e-12
    assert torch.equal(model.discrete_graph_learning.fc.weight.detach(), ckpt["model_state_dict"]["discrete_graph_learning.fc.weight"])
    state = ckpt["optim_state_dict"]["state"]
    for i, (name, off, p) in opt._index.items():
        assert float(state[i]["step"]) == 3.0
        assert torch.equal(opt.exp_avg[off:off + p.numel()].view(p.shape), state[i]["exp_avg"]), name
        assert torch.equal(opt.exp_avg_sq[off:off + p.numel()].view(p.shape), state[i]["exp_avg_sq"]), name
    assert sorted(opt._index) == sorted(state) and any(tuple(p.shape) == (100, 16 * T2) for _, _, p in opt._index.values())
    hist, long_hist, fut = (t.to(dev) for t in prob.batch(sorted(prob.train_t[:2])))
    path = runner.train_epoch(2, [(fut, hist, long_hist)])          # and the run goes on, and saves through the same save_model
    runner.flush_meters()
    assert opt.step_count == 4 and os.path.isfile(path)
    assert all(torch.isfinite(v).all() for v in model.state_dict().values())


def test_a_checkpoint_resumes_in_every_direction_and_continues_like_the_uninterrupted_run(tmp_path):
    run_two_ranks("shard_runner_worker.py", "resume", tmp_path, timeout=300)
