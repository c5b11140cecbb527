"""The pre-training tail on the device: libstep_hip step_pretrain_tail (loss, its gradient in the layout of the decoder's output and the
three training meters, from the decoder's output and the packed series in place) against the reference's own numbers
(tests/golden/pretrain_tail_cases.npz, recorded by tools/make_pretrain_tail_golden.py), its work buffer, its agreement with the existing
native path, ``TSFormer.pretrain_tail`` end to end on tests/golden/tsformer_pretrain_tiny.npz (also through a ``LongHistoryRef``), and
``native_runner(..., native_pretrain=True)`` against ``native_pretrain=False`` around one module.
Tolerances are the project's for these quantities (tests/test_gpu_train_tail.py:5-6): loss rel 1e-5, gradients rel_l2 < 1e-5, metrics
rtol 2e-5 / atol 1e-6; end to end the bounds of test_pretrain_matches_reference.  Host side: tests/test_pretrain_tail_host.py."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from tests.helpers import load_golden, max_abs, rel_l2
from tests.runner_double import RunnerDouble, masked_mae

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain_tail_cases.npz")
CASES = ("a", "b", "c", "d", "e", "e_un")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def device_case(c):
    z = fixture()
    return {key: torch.from_numpy(z[f"{c}.{key}"]).cuda() for key in ("r", "series", "mk")}


def run(c, grad_scale=None, retain=False, no_grad=False):
    """-> (loss, metrics, dr [S, P, 12] or None) of case c on the device"""
    from step_amd.step_arch.tsformer import _PretrainTail
    z, d = fixture(), device_case(c)
    r = d["r"].clone().requires_grad_(not no_grad)
    loss, metrics = _PretrainTail.apply(r, d["series"], d["mk"], 0.0, float(z[f"{c}.scale"]), float(z[f"{c}.shift"]), not no_grad)
    assert not metrics.requires_grad and metrics.dtype == torch.float32 and metrics.shape == (3,)
    if no_grad:
        assert not loss.requires_grad
        return loss, metrics, None
    out = loss if grad_scale is None else grad_scale * loss
    dr, = torch.autograd.grad(out, [r], retain_graph=retain)
    if retain:
        dr2, = torch.autograd.grad(out, [r])
        assert torch.equal(dr, dr2)          # the backward does not scale its saved gradient in place
    return loss.detach(), metrics, dr


@functools.lru_cache(maxsize=None)
def result(c):
    return run(c)


def masked_label_elements(c):
    """bool [S, P, 12]: the elements of the masked rows whose label is null after rescaling"""
    z = fixture()
    S, P, _ = z[f"{c}.r"].shape
    Pu, mk = int(z[f"{c}.Pu"]), z[f"{c}.mk"].astype(np.int64)
    y = torch.from_numpy(z[f"{c}.series"].reshape(S, P, 12)[:, mk, :]) * float(z[f"{c}.scale"]) + float(z[f"{c}.shift"])      # f32: multiply, then add
    out = torch.zeros(S, P, 12, dtype=torch.bool)
    out[:, Pu:, :] = torch.isclose(y, torch.zeros_like(y), atol=5e-5, rtol=0.0)
    return out


@pytest.mark.parametrize("c", CASES)
def test_every_case_against_the_reference(c):
    z = fixture()
    loss, metrics, dr = result(c)
    print(c, "loss", float(loss), float(z[f"{c}.loss"]), "metrics", metrics.tolist(), z[f"{c}.metrics"].tolist())
    assert float(loss) == pytest.approx(float(z[f"{c}.loss"]), rel=1e-5)
    assert torch.allclose(metrics.cpu(), torch.from_numpy(z[f"{c}.metrics"]), rtol=2e-5, atol=1e-6)
    dr, Pu = dr.cpu(), int(z[f"{c}.Pu"])
    nan_at = torch.isnan(torch.from_numpy(z[f"{c}.r"]))
    assert dr.shape == z[f"{c}.r"].shape and torch.isfinite(dr).all()
    assert (dr[:, :Pu] == 0).all()                                # the unmasked rows: written, and exactly zero
    assert (dr[masked_label_elements(c)] == 0).all()
    assert (dr[nan_at] == 0).all() and int(nan_at.sum()) == (1 if c in ("e", "e_un") else 0)
    want = torch.from_numpy(z[f"{c}.dr"])
    want[nan_at] = 0.0                                            # (the reference's gradient of a NaN term is NaN; here it is defined as 0)
    if float(want.abs().max()) == 0.0:                            # everything masked (case d)
        assert c == "d" and float(dr.abs().max()) == 0.0 and float(loss) == 0.0 and metrics.tolist() == [0.0, 0.0, 0.0]
    else:
        print(c, "rel_l2 dr", rel_l2(dr, want))
        assert rel_l2(dr, want) < 1e-5


def test_a_nan_in_an_unmasked_row_changes_nothing():
    for x, y in zip(result("b"), result("e_un")):
        assert torch.equal(x, y)


def test_work_buffer_is_left_clean_and_is_per_stream():
    from step_amd.step_arch import tsformer as T
    first = run("c")
    for i in range(3):                                            # an odd number of further calls, another case in between
        run("b")
    again = run("c")
    after_odd = run("c")
    for x, y, w in zip(first, again, after_odd):
        assert torch.equal(x, y) and torch.equal(x, w)
    main = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    assert main in T._PT_TAIL_WORK
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run("c")
        key = (torch.cuda.current_device(), side.cuda_stream)
    side.synchronize()
    assert key != main and key in T._PT_TAIL_WORK and T._PT_TAIL_WORK[key].data_ptr() != T._PT_TAIL_WORK[main].data_ptr()
    for x, y in zip(first, other):
        assert torch.equal(x, y)


@pytest.mark.parametrize("retain", (False, True))
def test_gradient_of_twice_the_loss_is_twice_the_gradient(retain):
    _, _, dr = result("b")
    _, _, dr2 = run("b", grad_scale=2.0, retain=retain)
    assert torch.equal(dr2, 2.0 * dr) and float(dr.abs().max()) > 0          # (a factor of two is exact in f32)


@pytest.mark.parametrize("c", ("a", "c", "e"))
def test_values_only_call_gives_the_same_bits(c):
    loss, metrics, _ = result(c)
    vloss, vmetrics, _ = run(c, no_grad=True)
    assert torch.equal(loss, vloss) and torch.equal(metrics, vmetrics)


def test_agrees_with_the_existing_native_path_on_case_c():
    """the views ``forward()`` cuts from r and the series (tsformer.py:152-158), masked_mae_native and masked_metrics_native on them"""
    from step_amd.step_loss import masked_mae_native, masked_metrics_native
    z, d = fixture(), device_case("c")
    mean, std = float(z["c.shift"]), float(z["c.scale"])
    B, N, Pu = int(z["c.B"]), int(z["c.N"]), int(z["c.Pu"])
    r = d["r"].clone().requires_grad_(True)
    P = r.shape[1]
    recon = r.view(B, N, P, 12)[:, :, Pu:, :].reshape(B, N, -1).transpose(1, 2)
    label = d["series"].view(B, N, P, 12)[:, :, d["mk"].long(), :].reshape(B, N, -1).transpose(1, 2)
    old = masked_mae_native(recon.transpose(1, 2), label.transpose(1, 2), rescale=(mean, std))
    odr, = torch.autograd.grad(old, [r])
    om = masked_metrics_native(recon.detach() * std + mean, label * std + mean, 0.0)
    loss, metrics, dr = result("c")
    print("loss", float(loss), float(old.detach()), "metrics", metrics.tolist(), om.tolist(), "rel_l2 dr", rel_l2(dr, odr))
    assert float(loss) == pytest.approx(float(old.detach()), rel=1e-5)
    assert torch.allclose(metrics, om, rtol=2e-5, atol=1e-6)
    assert rel_l2(dr, odr) < 1e-5


# ---------------------------------------------------------------------------------------------- the module, end to end
def tiny_model(g=None):
    from tests.test_gpu_pretrain import _model
    g = g or load_golden("tsformer_pretrain_tiny")
    model = _model(g, g["in.x"].shape[1])
    model.train()
    model.dropout_p = 0.0
    um, mk = g["in.unmasked"].tolist(), g["in.masked"].tolist()
    model.mask.forward = lambda: (um, mk)
    return g, model


def long_history_ref(x):
    """a LongHistoryRef over a device series that holds the windows x [B, L, N, C] one after the other"""
    from step_amd.step_arch.step import LongHistoryRef
    B, L = x.shape[:2]
    data = torch.cat(list(x), dim=0).contiguous()                 # [B * L, N, C]: window b is rows b L .. (b + 1) L - 1
    t0 = torch.arange(1, B + 1, dtype=torch.int64, device=x.device) * L
    return LongHistoryRef(data, t0, L, t0_host=t0.tolist())


def test_pretrain_tail_end_to_end_matches_the_reference():
    g, model = tiny_model()
    x = g["in.x"].cuda()
    loss, metrics = model.pretrain_tail(x, 0.0, rescale=(200.0, 150.0))
    assert loss.requires_grad and not metrics.requires_grad
    print("loss", float(loss.detach()), float(g["out.loss"]), "metrics", metrics.tolist())
    assert float(loss) == pytest.approx(float(g["out.loss"]), rel=1e-4)
    assert float(metrics[0]) == float(loss)
    loss.backward()
    torch.cuda.synchronize()
    worst, n = 0.0, 0
    for name, prm in model.named_parameters():
        want = g.get("grad." + name)
        if want is None:
            continue
        assert prm.grad is not None, name
        if float(want.abs().max()) < 1e-5:
            assert max_abs(prm.grad.cpu(), want) < 1e-4, name
            continue
        err = rel_l2(prm.grad.cpu(), want)
        worst = max(worst, err)
        assert err < 5e-3, (name, err)
        n += 1
    print("checked", n, "gradients, worst rel-L2", worst)
    assert n > 50
    # the same windows through a LongHistoryRef: one gather launch instead of the [B, L, N, C] tensor and the pack launch
    ref = long_history_ref(x)
    loss_ref, metrics_ref = model.pretrain_tail(ref, 0.0, rescale=(200.0, 150.0))
    assert float(loss_ref) == pytest.approx(float(loss), rel=1e-5)
    assert torch.allclose(metrics_ref, metrics, rtol=2e-5, atol=1e-6)
    with torch.no_grad():
        vloss, vmetrics = model.pretrain_tail(x, 0.0, rescale=(200.0, 150.0))
    assert not vloss.requires_grad and float(vloss) == pytest.approx(float(loss), rel=1e-5)
    # forward() is what it was, and takes the reference as well
    recon, label = model(history_data=x, future_data=None, batch_seen=0, epoch=1)
    recon_ref, label_ref = model(history_data=ref, future_data=None, batch_seen=0, epoch=1)
    assert max_abs(label.cpu(), g["out.label"]) == 0.0 and torch.equal(label_ref, label)
    assert recon_ref.shape == recon.shape == g["out.recon"].shape and max_abs(recon_ref, recon) < 2e-4
    # a reference that exposes another channel first reads that channel
    two = torch.cat([torch.zeros_like(ref.data), ref.data], dim=2)
    from step_amd.step_arch.step import LongHistoryRef
    _, label_ch = model(history_data=LongHistoryRef(two, ref.t0, ref.length)[:, :, :, [1]], future_data=None, batch_seen=0, epoch=1)
    assert torch.equal(label_ch, label)


# ---------------------------------------------------------------------------------------------- the runner
class PretrainRunnerDouble(RunnerDouble):
    """``TSFormerRunner.forward`` (step/step_runner/tsformer_runner.py:43-71), the base class's ``val_iters``
    (basicts/runners/base_tsf_runner.py:257-273) and what ``init_training`` leaves behind for step/TSFormer_PEMS04.py:52-73, restated
    on top of RunnerDouble"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.forward_features = [0]
        self.target_features = [0]
        self.val_base_calls = 0

    def forward(self, data, epoch=None, iter_num=None, train=True, **kwargs):
        future_data, history_data = data
        history_data = self.to_running_device(history_data)
        future_data = self.to_running_device(future_data)
        batch_size, length, num_nodes, _ = future_data.shape
        history_data = self.select_input_features(history_data)
        return self.model(history_data=history_data, future_data=None, batch_seen=iter_num, epoch=epoch)

    def val_iters(self, iter_index, data):
        self.val_base_calls += 1
        forward_return = self.forward(data=data, epoch=None, iter_num=None, train=False)
        mean, std = self.scaler["args"]["mean"], self.scaler["args"]["std"]
        prediction_rescaled, real_value_rescaled = forward_return[0] * std + mean, forward_return[1] * std + mean
        for metric_name, metric_func in self.metrics.items():
            metric_item = self.metric_forward(metric_func, [prediction_rescaled, real_value_rescaled])
            self.update_epoch_meter("val_" + metric_name, metric_item.item())

    def init_training(self, cfg):
        self.optim = torch.optim.Adam(self.model.parameters(), **cfg["TRAIN"]["OPTIM"]["PARAM"])
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optim, **cfg["TRAIN"]["LR_SCHEDULER"]["PARAM"])
        self.clip_grad_param = dict(cfg["TRAIN"]["CLIP_GRAD_PARAM"])


@functools.lru_cache(maxsize=None)
def runner_problem():
    """one module (dropout off) and two batches (future, history); one sensor reads a raw 0.0, masked after rescaling"""
    from tests.test_gpu_pretrain import _model
    g = load_golden("tsformer_pretrain_tiny")
    model = _model(g, g["in.x"].shape[1])
    model.train()
    model.dropout_p = 0.0
    x = g["in.x"].cuda().clone()
    x[:, :, 0, 0] = -200.0 / 150.0
    x2 = (x.flip(0) * 0.9 + 0.05).contiguous()
    fut = torch.zeros(x.shape[0], 12, x.shape[2], 1, device="cuda")
    return model, [(fut, x), (fut, x2)]


def iterations(native_pretrain, loss_fn=masked_mae, batches=None):
    """two training iterations (no optimizer step: the same weights on both sides), one validation iteration, one flush"""
    from step_amd.runner import native_runner
    model, data = runner_problem()
    runner = native_runner(PretrainRunnerDouble, native_pretrain=native_pretrain)(
        {"model": model, "loss": loss_fn, "scaler": (200.0, 150.0), "cl": None})
    losses, grads = [], []
    for it, batch in enumerate(data if batches is None else batches(data)):
        random.seed(1234 + it)                                    # the same masks on both sides
        model.zero_grad(set_to_none=True)
        loss = runner.train_iters(1, it, batch)
        loss.backward()
        grads.append(model._flat_grad.clone())
        losses.append(float(loss))
    random.seed(99)
    with torch.no_grad():
        runner.val_iters(0, (data if batches is None else batches(data))[0])
    pending = {k: len(v) for k, v in runner._pending.items()}
    runner.flush_meters()
    meters = {k: runner.meters[k].avg for k in runner.meters}
    assert sorted(meters) == sorted(p + k for p in ("train_", "val_") for k in ("MAE", "RMSE", "MAPE"))
    assert all(runner.meters["train_" + k].n == 2 and runner.meters["val_" + k].n == 1 for k in ("MAE", "RMSE", "MAPE"))
    return losses, meters, grads, runner, pending


def test_runner_native_pretrain_equals_the_base_class_path():
    """parameter gradients: two native backwards sum with f32 atomics, relative L2 1e-3 as in tests/test_gpu_train_tail.py"""
    l0, m0, g0, r0, _ = iterations(False)
    l1, m1, g1, r1, pending = iterations(True)
    print("losses", l0, l1, "meters", m0, m1, "relative L2 of the flat gradients", [float((a - b).norm() / b.norm()) for a, b in zip(g1, g0)])
    assert r0.base_calls == 2 and r0.val_base_calls == 1
    assert r1.base_calls == 0 and r1.val_base_calls == 0          # neither went through the base class's train_iters / val_iters
    assert pending == {p + k: n for p, n in (("train_", 2), ("val_", 1)) for k in ("MAE", "RMSE", "MAPE")}      # nothing was read back per iteration
    for a, b in zip(l1, l0):
        assert a == pytest.approx(b, rel=2e-5)
    for k in m0:
        assert m1[k] == pytest.approx(m0[k], rel=2e-5), k
    assert m0["train_MAE"] == pytest.approx(sum(l0) / 2, rel=2e-5) and l0[0] != l0[1]
    for a, b in zip(g1, g0):
        assert float(b.norm()) > 0 and float((a - b).norm() / b.norm()) <= 1e-3


def test_runner_native_pretrain_takes_a_long_history_ref():
    l0, m0, _, _, _ = iterations(True)
    l1, m1, _, r1, _ = iterations(True, batches=lambda data: [(f, long_history_ref(x)) for f, x in data])
    assert r1.base_calls == 0 and r1.val_base_calls == 0
    for a, b in zip(l1, l0):
        assert a == pytest.approx(b, rel=1e-5)
    for k in m0:
        assert m1[k] == pytest.approx(m0[k], rel=2e-5), k


def test_runner_keeps_the_base_path_for_another_loss():
    def my_loss(*args, **kwargs):
        return masked_mae(*args, **kwargs)
    l0, m0, _, r0, _ = iterations(False, loss_fn=my_loss)
    l1, m1, _, r1, _ = iterations(True, loss_fn=my_loss)
    assert r0.base_calls == 2 and r1.base_calls == 2 and r1.val_base_calls == 1
    assert l1 == pytest.approx(l0, rel=1e-5) and m1 == pytest.approx(m0, rel=2e-5)


def test_init_training_leaves_a_fused_optimizer_and_the_state_dict_keys():
    from step_amd.optim import FusedAdamClip
    from step_amd.runner import native_runner
    g, model = tiny_model()
    keys = list(model.state_dict())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    cfg = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 0.001, "weight_decay": 0, "eps": 1.0e-8, "betas": (0.9, 0.95)}},
                     "LR_SCHEDULER": {"PARAM": {"milestones": [50], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 5.0}}}
    plain = native_runner(PretrainRunnerDouble)({"model": model, "loss": masked_mae, "scaler": (200.0, 150.0), "cl": None})
    plain.init_training(cfg)
    assert type(plain.optim) is torch.optim.Adam and plain.clip_grad_param == {"max_norm": 5.0} and model._flat_param is None
    runner = native_runner(PretrainRunnerDouble, native_pretrain=True)({"model": model, "loss": masked_mae, "scaler": (200.0, 150.0), "cl": None})
    runner.init_training(cfg)
    assert isinstance(runner.optim, FusedAdamClip) and runner.clip_grad_param is None and runner.optim.max_norm == 5.0
    assert runner.optim.param_groups[0]["lr"] == 0.001 and runner.optim.param_groups[0]["betas"] == (0.9, 0.95)
    assert isinstance(runner.scheduler, torch.optim.lr_scheduler.MultiStepLR) and runner.scheduler.optimizer is runner.optim
    assert model._flat_param is not None and list(model.state_dict()) == keys
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    # one step of the reference's loop: zero_grad, train_iters, backward, step
    runner.optim.zero_grad()
    loss = runner.train_iters(1, 0, (torch.zeros(2, 12, 9, 1, device="cuda"), g["in.x"].cuda()))
    loss.backward()
    runner.optim.step()
    runner.scheduler.step()
    after = model.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert not torch.equal(after["output_layer.weight"], before["output_layer.weight"])
