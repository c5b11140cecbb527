"""The training tail on the device: ``step_amd.step_loss.train_tail`` (libstep_hip step_train_tail: loss, both gradients and the three
training meters on the first k horizon steps, from the normalised prediction and the batch's label view) against the reference's own
numbers (tests/golden/train_tail_cases.npz, recorded by tools/make_train_tail_golden.py), its work buffer, its agreement with the
existing native path, and ``native_runner(..., native_tail=True)`` against ``native_tail=False`` around one module.
Tolerances are the project's for these quantities (tests/test_gpu_step.py:372-375, 438): loss rel 1e-5, gradients rel_l2 < 1e-5,
metrics rtol 2e-5 / atol 1e-6.  Host side: tests/test_train_tail_host.py."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_tail_cases.npz")
KS = (1, 5, 11, 12)
CASES = ("a", "b", "c", "d", "e0", "e11")


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def device_case(c):
    z = fixture()
    return {key: torch.from_numpy(z[f"{c}.{key}"]).cuda() for key in ("pred", "real", "theta", "prior")}


def run(c, k, label="view", grad_scale=None, retain=False, via_loss=False):
    """-> (loss, metrics, dpred [B, 12, N], dtheta) of case c on the device"""
    from step_amd.step_loss import step_loss_native, train_tail
    z, d = fixture(), device_case(c)
    pred = d["pred"][..., None].clone().requires_grad_(True)
    theta = d["theta"].clone().requires_grad_(True)
    real = d["real"][..., :1]                                  # channel 0 of [B, 12, N, C], in place
    if label == "contiguous":
        real = real.contiguous()
    elif label == "indexed":
        real = d["real"][..., [0]]
    kw = dict(null_val=0.0, rescale=(float(z[f"{c}.shift"]), float(z[f"{c}.scale"])), horizons=k)
    if via_loss:
        loss, metrics = step_loss_native(pred, real, theta, d["prior"], float(z[f"{c}.coef"]), **kw), None
    else:
        loss, metrics = train_tail(pred, real, theta, d["prior"], float(z[f"{c}.coef"]), **kw)
        assert not metrics.requires_grad and metrics.dtype == torch.float32 and metrics.shape == (3,)
    out = loss if grad_scale is None else grad_scale * loss
    dp, dt = torch.autograd.grad(out, [pred, theta], retain_graph=retain)
    if retain:
        dp2, dt2 = torch.autograd.grad(out, [pred, theta])
        assert torch.equal(dp, dp2) and torch.equal(dt, dt2)          # the backward does not scale its saved gradients in place
    return loss.detach(), metrics, dp[..., 0], dt


@functools.lru_cache(maxsize=None)
def result(c, k):
    return run(c, k)


def masked_labels(c):
    z = fixture()
    y = torch.from_numpy(z[f"{c}.real"][..., 0]) * float(z[f"{c}.scale"]) + float(z[f"{c}.shift"])          # f32: multiply, then add
    return torch.isclose(y, torch.zeros_like(y), atol=5e-5, rtol=0.0)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("c", CASES)
def test_every_case_and_k_against_the_reference(c, k):
    z = fixture()
    loss, metrics, dp, dt = result(c, k)
    print(c, k, "loss", float(loss), float(z[f"{c}.{k}.loss"]), "metrics", metrics.tolist(), z[f"{c}.{k}.metrics"].tolist())
    assert float(loss) == pytest.approx(float(z[f"{c}.{k}.loss"]), rel=1e-5)
    assert torch.allclose(metrics.cpu(), torch.from_numpy(z[f"{c}.{k}.metrics"]), rtol=2e-5, atol=1e-6)
    dp = dp.cpu()
    assert (dp[:, k:] == 0).all()                              # excluded horizons: written, and exactly zero
    assert (dp[masked_labels(c)] == 0).all()
    assert torch.isfinite(dp).all()
    assert rel_l2(dt.cpu(), torch.from_numpy(z[f"{c}.dtheta"])) < 1e-5
    if f"{c}.{k}.dpred" in z:
        want = torch.from_numpy(z[f"{c}.{k}.dpred"])
        print(c, k, "rel_l2 dpred", rel_l2(dp, want) if float(want.abs().max()) else "all-zero")
        if float(want.abs().max()) == 0.0:                     # everything masked (case d, k <= 5)
            assert float(dp.abs().max()) == 0.0
        else:
            assert rel_l2(dp, want) < 1e-5
    else:                                                      # an included NaN prediction: values only; its own gradient is defined as 0
        nan_at = torch.isnan(torch.from_numpy(z[f"{c}.pred"]))
        assert c in ("e0", "e11") and int(nan_at[:, :k].sum()) == 1 and (dp[nan_at] == 0).all()


@pytest.mark.parametrize("k", (1, 5, 11))
def test_an_excluded_nan_prediction_changes_nothing(k):
    a, e = result("a", k), result("e11", k)
    for x, y in zip(a, e):
        assert torch.equal(x, y)


def test_all_masked_slice_leaves_the_graph_term():
    z = fixture()
    for k in (1, 5):
        loss, metrics, dp, dt = result("d", k)
        assert metrics.tolist() == [0.0, 0.0, 0.0] and float(dp.abs().max()) == 0.0
        assert float(loss) == pytest.approx(float(z[f"d.{k}.loss"]), rel=1e-5) and float(loss) > 0


@pytest.mark.parametrize("c,k", [("b", 5), ("c", 12), ("c", 1)])
def test_label_view_and_its_copies_give_identical_bits(c, k):
    base = result(c, k)
    for label in ("contiguous", "indexed"):
        for x, y in zip(base, run(c, k, label=label)):
            assert torch.equal(x, y), label


def test_work_buffer_is_left_clean_and_is_per_stream():
    from step_amd import step_loss as SL
    first = run("c", 12)
    for i in range(3):                                         # an odd number of further calls, another case in between
        run("b", 5)
    again = run("c", 12)
    after_odd = run("c", 12)
    for x, y, w in zip(first, again, after_odd):
        assert torch.equal(x, y) and torch.equal(x, w)
    main = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    assert main in SL._TAIL_WORK
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run("c", 12)
        key = (torch.cuda.current_device(), side.cuda_stream)
    side.synchronize()
    assert key != main and key in SL._TAIL_WORK and SL._TAIL_WORK[key].data_ptr() != SL._TAIL_WORK[main].data_ptr()
    for x, y in zip(first, other):
        assert torch.equal(x, y)


@pytest.mark.parametrize("c", CASES)
def test_all_horizons_agree_with_the_existing_native_path(c):
    from step_amd.step_loss import masked_metrics_native, step_loss_native
    z, d = fixture(), device_case(c)
    mean, std = float(z[f"{c}.shift"]), float(z[f"{c}.scale"])
    pred = d["pred"][..., None].clone().requires_grad_(True)
    theta = d["theta"].clone().requires_grad_(True)
    real = d["real"][..., :1]
    old = step_loss_native(pred, real, theta, d["prior"], float(z[f"{c}.coef"]), null_val=0.0, rescale=(mean, std))
    odp, odt = torch.autograd.grad(old, [pred, theta])
    om = masked_metrics_native(pred.detach() * std + mean, real * std + mean, 0.0)
    loss, metrics, dp, dt = result(c, 12)
    assert float(loss) == pytest.approx(float(old.detach()), rel=1e-5)          # (finite for d, e0 and e11 as well: nan never equals nan)
    assert rel_l2(dp, odp[..., 0]) < 1e-5 and rel_l2(dt, odt) < 1e-5
    assert torch.equal(dp != 0, odp[..., 0] != 0)                          # the same labels masked, the same NaN terms without a gradient
    assert torch.allclose(metrics, om, rtol=2e-5, atol=1e-6)
    none = run(c, None)                                        # horizons=None: all of them
    for x, y in zip(none, (loss, metrics, dp, dt)):
        assert torch.equal(x, y)
    via = run(c, 5, via_loss=True)                             # step_loss_native(..., horizons=k) is train_tail's loss
    five = result(c, 5)
    assert torch.equal(via[0], five[0]) and torch.equal(via[2], five[2]) and torch.equal(via[3], five[3])


@pytest.mark.parametrize("retain", (False, True))
def test_gradient_of_twice_the_loss_is_twice_the_gradient(retain):
    _, _, dp, dt = result("b", 5)
    _, _, dp2, dt2 = run("b", 5, grad_scale=2.0, retain=retain)
    assert torch.equal(dp2, 2.0 * dp) and torch.equal(dt2, 2.0 * dt)          # (a factor of two is exact in f32)
    assert float(dp.abs().max()) > 0 and float(dt.abs().max()) > 0


@pytest.mark.parametrize("k", (0, 13))
def test_bad_horizons_raise(k):
    from step_amd.step_loss import step_loss_native, train_tail
    d = device_case("a")
    args = (d["pred"][..., None], d["real"][..., :1], d["theta"], d["prior"], 1.0)
    with pytest.raises(ValueError):
        train_tail(*args, horizons=k)
    with pytest.raises(ValueError):
        step_loss_native(*args, horizons=k)


# ---------------------------------------------------------------------------------------------- the runner
@functools.lru_cache(maxsize=None)
def tiny():
    """a step_tiny module in f32 mode, dropout off, fixed Gumbel noise, and one batch (future, history, long history)"""
    from tests.test_gpu_step import build_native, inputs_of
    g = load_golden("step_tiny")
    model = build_native(g)
    model.train()
    model.matmul_precision = "f32"
    model.backend.dropout = 0.0
    model.tsformer.dropout_p = 0.0
    model._noise_override = g["in.u"]
    hist, long_hist, fut = inputs_of(g)
    fut = fut.clone()
    fut[:, :, 0, 0] = -float(g["meta.scaler"][0]) / float(g["meta.scaler"][1])          # one sensor reads a raw 0.0: masked after rescaling
    return g, model, (fut, hist, long_hist)


def one_iteration(native_tail, cl, epoch, loss_fn=None):
    from step_amd.runner import native_runner
    from step_amd.step_loss import step_loss_native
    from tests.runner_double import RunnerDouble
    g, model, batch = tiny()
    mean, std = [float(x) for x in g["meta.scaler"]]
    runner = native_runner(RunnerDouble, native_tail=native_tail)(
        {"model": model, "loss": loss_fn or step_loss_native, "scaler": (mean, std), "cl": cl})
    model.zero_grad(set_to_none=True)
    loss = runner.train_iters(epoch, 0, batch)
    loss.backward()
    grad = model._flat_grad.clone()
    runner.flush_meters()
    meters = {k: runner.meters["train_" + k].avg for k in ("MAE", "RMSE", "MAPE")}
    assert all(runner.meters["train_" + k].n == 1 for k in meters) and list(runner.meters) == ["train_MAE", "train_RMSE", "train_MAPE"]
    return float(loss), meters, grad, runner


CL = {"WARM_EPOCHS": 0, "CL_EPOCHS": 1, "PREDICTION_LENGTH": 12}


@pytest.mark.parametrize("cl,epoch", [(CL, 1), (CL, 5), (CL, 12), (None, 1)])
def test_runner_native_tail_equals_the_base_class_tail(cl, epoch):
    """same module, same batch, same weights (no optimizer step is taken): one iteration with the tail on torch ops and the existing
    kernels (native_tail=False) and one with train_tail.  Parameter gradients: two native backwards sum with f32 atomics, relative L2
    1e-3 as in tests/test_gpu_eval_cache.py."""
    l0, m0, g0, r0 = one_iteration(False, cl, epoch)
    l1, m1, g1, r1 = one_iteration(True, cl, epoch)
    rel = float((g1 - g0).norm() / g0.norm())
    print("cl", cl is not None, "epoch", epoch, "loss", l0, l1, "meters", m0, m1, "relative L2 of the flat gradients", rel)
    assert r0.base_calls == 1 and r1.base_calls == 0          # the second one did not go through the base class's train_iters
    if cl is not None:
        assert r1.curriculum_learning(epoch) == epoch
    assert l1 == pytest.approx(l0, rel=1e-5)
    for k in m0:
        assert m1[k] == pytest.approx(m0[k], rel=2e-5)
    assert float(g0.norm()) > 0 and rel <= 1e-3


def test_runner_keeps_the_base_path_for_another_loss():
    from step_amd.step_loss import step_loss_native

    def my_loss(*args, **kwargs):
        return step_loss_native(*args, **kwargs)
    l0, m0, _, r0 = one_iteration(False, CL, 5, loss_fn=my_loss)
    l1, m1, _, r1 = one_iteration(True, CL, 5, loss_fn=my_loss)
    assert r0.base_calls == 1 and r1.base_calls == 1
    assert l1 == pytest.approx(l0, rel=1e-5) and m1 == pytest.approx(m0, rel=2e-5)
