"""Gradient accumulation, host side (no GPU): the group logic of ``native_runner(..., accumulate=k)`` against doubles of the
easytorch loop (group sizes with the short last group, the 1 / s loss scale, the order of zero_grad / backward / step, the raise when
the fused optimizer is absent), ``FusedAdamClip``'s count check with the library call stubbed, and the argument / state rules of
``set_grad_accumulation`` on both modules.  The kernels and the modules on the device: tests/test_gpu_grad_accum.py."""
import inspect

import pytest
import torch

from step_amd.optim import FusedAdamClip
from step_amd.runner import native_runner


# ---------------------------------------------------------------------------------------------- the runner's groups
class _Model(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(()))
        self.log = log

    def set_grad_accumulation(self, k):
        self.log.append(("set", k))


class _Fused(FusedAdamClip):
    """an instance of the fused optimizer's type that only records (no flat buffer, no library)"""

    def __init__(self, model, log):
        self.model, self.log = model, log

    def zero_grad(self, set_to_none=True):
        self.log.append(("zero_grad",))
        self.model.w.grad = None

    def step(self, closure=None):
        self.log.append(("step", float(self.model.w.grad)))


class _Base:
    """easytorch's loop around the hooks the native runner overrides: ``backward`` is zero_grad -> backward -> (clip) -> step"""

    def __init__(self, cfg):
        self.log = cfg["log"]
        self.model = _Model(self.log)
        self.fused = cfg.get("fused", True)
        self.train_data_loader = list(cfg["data"])
        self.optim = self.scheduler = None
        self.clip_grad_param = None
        self.metrics = {}

    def build_train_data_loader(self, cfg):
        return None

    def init_training(self, cfg):
        self.optim = _Fused(self.model, self.log) if self.fused else torch.optim.Adam(self.model.parameters())

    def train_iters(self, epoch, iter_index, data):
        self.log.append(("forward", iter_index))
        return self.model.w * data          # d loss / d w = data

    def backward(self, loss):
        self.log.append(("base_backward",))
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()

    def epoch(self, epoch=1):
        for it, data in enumerate(self.train_data_loader):
            loss = self.train_iters(epoch, it, data)
            self.backward(loss)
            self.log.append(("iteration_done", it, float(loss.detach())))


def _run(data, k, **kw):
    log = []
    runner = native_runner(_Base, accumulate=k, **kw)({"log": log, "data": data})
    runner.init_training({})
    runner.epoch()
    return log, runner


def test_the_switches_exist_and_default_to_today():
    from step_amd import STEP, TSFormer
    assert inspect.signature(native_runner).parameters["accumulate"].default == 1
    assert list(inspect.signature(STEP.set_grad_accumulation).parameters) == ["self", "k"]
    assert list(inspect.signature(TSFormer.set_grad_accumulation).parameters) == ["self", "k"]
    from step_amd import _lib
    assert "step_dgl_edges_backward_acc" in _lib.exported_symbols() and _lib.ABI_VERSION == 10
    for bad in (0, -2, 1.0, True, "2", None):
        with pytest.raises((ValueError, TypeError)):
            native_runner(_Base, accumulate=bad)


def test_accumulate_one_is_the_base_class_loop():
    log, runner = _run([1.0, 2.0, 3.0], 1)
    per_iter = [("forward", 0), ("base_backward",), ("zero_grad",), ("step", 1.0), ("iteration_done", 0, 0.0)]
    assert log[:5] == per_iter and len(log) == 15
    assert not any(e[0] == "set" for e in log)          # the module is not told anything
    assert [e[1] for e in log if e[0] == "step"] == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("n,k", [(4, 2), (5, 2), (7, 3), (2, 4), (1, 3), (6, 6)])
def test_groups_sizes_loss_scale_and_order(n, k):
    data = [float(2 ** i) for i in range(n)]          # powers of two: the sums below are exact in float32
    log, runner = _run(data, k)
    assert not any(e[0] == "base_backward" for e in log)
    sizes = [min(k, n - s) for s in range(0, n, k)]
    assert [e[1] for e in log if e[0] == "set"] == sizes          # the short last group is announced with its own size
    want, it = [], 0
    for s in sizes:
        want += [("zero_grad",), ("set", s)]          # before the group's first forward
        for j in range(s):
            want += [("forward", it), ("iteration_done", it, 0.0)]
            it += 1
        # the optimizer step after the group's last backward, on the sum of the group's gradients scaled by 1 / s
        want.insert(len(want) - 1, ("step", sum(data[it - s:it]) / s))
    # (the scaled gradients are float32: 1 / 3 is not exact, s + 1 roundings of 2^-24 each at the most)
    assert [e if e[0] != "step" else ("step",) for e in log] == [e if e[0] != "step" else ("step",) for e in want]
    assert [e[1] for e in log if e[0] == "step"] == pytest.approx([e[1] for e in want if e[0] == "step"], rel=(k + 1) * 2.0 ** -24)
    assert sum(1 for e in log if e[0] == "step") == len(sizes)


def test_meters_stay_per_iteration():
    """the loss train_iters returns (what easytorch's meters see) is the iteration's own, not the scaled one"""
    log, runner = _run([1.0, 2.0, 4.0], 2)
    runner.model.w.data.fill_(3.0)
    loss = runner.train_iters(1, 0, 5.0)
    assert float(loss) == 15.0


def test_accumulate_without_the_fused_optimizer_raises():
    log = []
    runner = native_runner(_Base, accumulate=2)({"log": log, "data": [1.0], "fused": False})
    with pytest.raises(RuntimeError, match="accumulate=2 needs the fused optimizer"):
        runner.init_training({})
    # with accumulate = 1 the same runner keeps torch's optimizer, as before
    runner = native_runner(_Base)({"log": log, "data": [1.0], "fused": False})
    runner.init_training({})
    assert type(runner.optim) is torch.optim.Adam


# ---------------------------------------------------------------------------------------------- the optimizer's count check
def _stub_library(monkeypatch):
    from step_amd import optim
    calls = []
    monkeypatch.setattr(optim._lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(optim._lib, "ptr", lambda t: None)
    monkeypatch.setattr(optim._lib, "stream", lambda: None)
    return calls


def _step_model():
    from tests.test_abi_and_host import _tiny_model
    return _tiny_model()[0]


def _pretrain_model():
    from step_amd import TSFormer
    return TSFormer(12, 1, 96, 4, 4, 0.1, 16, 0.75, 4, 1, mode="pre-train")


@pytest.mark.parametrize("make", [_step_model, _pretrain_model])
def test_fused_adam_clip_takes_exactly_k_backwards(monkeypatch, make):
    calls = _stub_library(monkeypatch)
    model = make()
    opt = FusedAdamClip(model, max_norm=3.0)
    model._flat_grad = torch.zeros_like(opt.flat)
    # k = 1: the message and the behaviour of before
    model._backward_count = 2
    with pytest.raises(RuntimeError, match="2 native backwards since zero_grad.. -- the flat gradient buffer holds the last one only"):
        opt.step()
    model.set_grad_accumulation(3)
    for count in (1, 2, 4):
        model._backward_count = count
        with pytest.raises(RuntimeError, match=f"{count} native backwards since zero_grad.., the model accumulates 3 per step"):
            opt.step()
    assert opt.step_count == 0 and calls == []
    model._backward_count = 3
    opt.step()
    assert opt.step_count == 1 and [c[0] for c in calls] == ["step_adam_clip_sharded"]
    assert calls[0][1][10] == 1          # the kernel's step number (bias correction): per optimizer step, not per micro-batch
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-3)          # 2e-3 halved after ONE scheduler step


@pytest.mark.parametrize("make", [_step_model, _pretrain_model])
def test_set_grad_accumulation_arguments_and_open_group(make):
    model = make()
    assert model._grad_accum == 1
    for bad in (0, -1):
        with pytest.raises(ValueError):
            model.set_grad_accumulation(bad)
    for bad in (1.5, 2.0, "2", None, True):
        with pytest.raises(TypeError):
            model.set_grad_accumulation(bad)
    model.set_grad_accumulation(4)
    assert model._grad_accum == 4
    model._group_open = True          # what a training forward that takes gradients leaves
    with pytest.raises(RuntimeError, match="group is open"):
        model.set_grad_accumulation(2)
    model.zero_grad()
    model.set_grad_accumulation(1)
    assert model._grad_accum == 1 and model._acc is None


def test_step_refuses_k_above_one_with_slices_or_a_captured_step(monkeypatch):
    model = _step_model()
    model.discrete_graph_learning._shard = {"world": 2}
    with pytest.raises(RuntimeError, match="time-sliced graph learner"):
        model.set_grad_accumulation(2)
    model.set_grad_accumulation(1)          # k = 1 is always fine
    model.discrete_graph_learning._shard = None
    model._dyn = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GraphedTrainStep"):
        model.set_grad_accumulation(2)
    model._dyn = None
    model.set_grad_accumulation(2)
    # ... and the other way round: a GraphedTrainStep is not built around an accumulating model
    _stub_library(monkeypatch)
    from step_amd.graphed import GraphedTrainStep
    opt = FusedAdamClip(model)
    with pytest.raises(RuntimeError, match="accumulate 2 micro-batches"):
        GraphedTrainStep(model, opt, (torch.zeros(1), torch.zeros(1), torch.zeros(1)))
    # a model that was sliced after k was set is refused at the first training forward of a group
    model.discrete_graph_learning._shard = {"world": 2}
    with pytest.raises(RuntimeError, match="time-sliced graph learner"):
        model._group_forward(0, 1, 100)


def test_group_rules_of_the_step_module_without_a_device():
    """the bookkeeping around the kept global feature: first forward opens, later ones reuse, a weight change makes it stale, the
    k-th backward is the last and a further one raises, zero_grad closes"""
    model = _step_model()
    model.set_grad_accumulation(2)
    bf, N, T = 0, model.backend.num_nodes, model.discrete_graph_learning.train_length
    grp = model._group_forward(bf, N, T)
    assert grp is model._acc and grp["fwd"] == 0 and grp["kept"] is None and model._group_open
    grp["kept"], grp["fwd"] = ("g", "gsaved"), 1          # what _StepFunction.forward leaves
    assert model._group_forward(bf, N, T) is grp
    with torch.no_grad():
        model.discrete_graph_learning.fc.weight.add_(1.0)          # a version bump: torch optimizers, user code
    with pytest.raises(RuntimeError, match="changed inside an accumulation group"):
        model._group_forward(bf, N, T)
    model.zero_grad()
    assert model._acc is None and not model._group_open
    grp = model._group_forward(bf, N, T)
    grp["kept"], grp["fwd"] = ("g", "gsaved"), 1
    model.load_state_dict(model.state_dict())
    assert grp["kept"] is None          # dropped, never reused
    with pytest.raises(RuntimeError, match="changed inside an accumulation group"):
        model._group_forward(bf, N, T)
    model.zero_grad()
    grp = model._group_forward(bf, N, T)
    grp["kept"], grp["fwd"] = ("g", "gsaved"), 2
    model.flat_gradients_only = True
    assert model._group_backward(grp) == (1, False)
    grp["bufs"] = ("flat", "views", "gw", "dg")
    model._drop_eval_g()
    assert grp["kept"] is not None          # a backward inside the group changes no weight
    assert model._group_backward(grp) == (2, True)
    model._drop_eval_g()          # what the optimizer step calls
    assert grp["kept"] is None
    with pytest.raises(RuntimeError, match="backward 3 of an accumulation group of 2"):
        model._group_backward(grp)
    model.zero_grad()
    with pytest.raises(RuntimeError, match="closed by zero_grad"):
        model._group_backward(grp)
