"""Host side of the training tail (``step_amd.step_loss.train_tail``, ``native_runner(..., native_tail=True)``): the fixture
tests/golden/train_tail_cases.npz is what the ORACLE's step_loss / rescale (pinned to the reference by tests/test_oracle_golden.py) and
the restated metrics give on the ``[:, :k]`` slices, the recording tool reproduces the stored file where the reference is at hand, the
runner keeps the base class's path where the native tail cannot run, and the library's work-buffer size needs no device.
Device side: tests/test_gpu_train_tail.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import step_oracle as O
from oracle.reference_loader import reference_root
from tests.test_abi_and_host import _DummyBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "train_tail_cases.npz")


def restated_metrics(p, y, null):
    """basicts/metrics/{mae,rmse,mape}.py as tests/test_gpu_step.py:415-427 restates them"""
    def mask_of(lab, nv):
        m = (~torch.isclose(lab, torch.tensor(nv).expand_as(lab), atol=5e-5, rtol=0.)).float()
        m = m / m.mean()
        return torch.where(torch.isnan(m), torch.zeros_like(m), m)
    m = mask_of(y, null)
    mae = torch.nan_to_num(torch.abs(p - y) * m, nan=0.0).mean()
    mse = torch.nan_to_num((p - y) ** 2 * m, nan=0.0).mean()
    y0 = torch.where(torch.abs(y) < 1e-4, torch.zeros_like(y), y)
    m0 = mask_of(y0, 0.0)
    ape = torch.abs(torch.abs(p - y0) / y0) * m0
    mape = torch.where(torch.isnan(ape), torch.zeros_like(ape), ape).mean()
    return torch.stack([mae, torch.sqrt(mse), mape])


def test_fixture_equals_the_oracle_on_the_slices():
    """same f32 operations on the same CPU: 1e-6 leaves room for the order of a sum only"""
    z = np.load(FIXTURE)
    assert z["ks"].tolist() == [1, 5, 11, 12] and sorted(z["cases"].tolist()) == ["a", "b", "c", "d", "e0", "e11"]
    assert os.path.getsize(FIXTURE) < 1 << 20
    for c in z["cases"].tolist():
        mean, std, coef = float(z[f"{c}.shift"]), float(z[f"{c}.scale"]), float(z[f"{c}.coef"])
        real = torch.from_numpy(z[f"{c}.real"])[..., :1]
        assert z[f"{c}.pred"].shape[1] == 12 and z[f"{c}.theta"].shape[1:] == (16, 16)
        for k in z["ks"].tolist():
            pred = torch.from_numpy(z[f"{c}.pred"])[..., None].clone().requires_grad_(True)
            theta = torch.from_numpy(z[f"{c}.theta"]).clone().requires_grad_(True)
            p, y = O.rescale(pred, mean, std)[:, :k], O.rescale(real, mean, std)[:, :k]
            loss = O.step_loss(p, y, theta, torch.from_numpy(z[f"{c}.prior"]), coef, null_val=0.0)
            dp, dt = torch.autograd.grad(loss, [pred, theta])
            assert float(loss.detach()) == pytest.approx(float(z[f"{c}.{k}.loss"]), rel=1e-6)
            np.testing.assert_allclose(restated_metrics(p.detach(), y, 0.0).numpy(), z[f"{c}.{k}.metrics"], rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(dt.numpy(), z[f"{c}.dtheta"], rtol=1e-6, atol=1e-9)
            if f"{c}.{k}.dpred" in z.files:
                want = z[f"{c}.{k}.dpred"]
                np.testing.assert_allclose(dp[..., 0].numpy(), want, rtol=1e-6, atol=1e-12)
                assert (want[:, k:] == 0).all()
            else:
                assert c in ("e0", "e11") and np.isnan(z[f"{c}.pred"][:, :k]).any()
    # d: nothing counts for k <= 5 -- the graph term alone, metrics 0; e11: the NaN is excluded for k < 12 and the results are case a's
    for k in (1, 5):
        assert z[f"d.{k}.metrics"].tolist() == [0.0, 0.0, 0.0] and (z[f"d.{k}.dpred"] == 0).all()
        assert float(z[f"d.{k}.loss"]) == float(z["d.1.loss"]) > 0
    for k in (1, 5, 11):
        assert z[f"e11.{k}.loss"] == z[f"a.{k}.loss"] and np.array_equal(z[f"e11.{k}.metrics"], z[f"a.{k}.metrics"])
        assert np.array_equal(z[f"e11.{k}.dpred"], z[f"a.{k}.dpred"])


@pytest.mark.skipif(reference_root() is None, reason="needs the reference sources")
def test_recording_tool_reproduces_the_stored_fixture():
    spec = importlib.util.spec_from_file_location("make_train_tail_golden", os.path.join(ROOT, "tools", "make_train_tail_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got, z = tool.compute(), np.load(FIXTURE)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        a, b = np.asarray(got[key]), z[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if key.split(".")[-1] in ("loss", "metrics", "dpred", "dtheta"):          # results: f32 sums on another CPU may be ordered differently
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-12, err_msg=key)
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


def test_native_tail_on_cpu_tensors_takes_the_base_path():
    """modelled on test_native_runner_hooks_on_the_host: no STEP module on a GPU, so ``native_tail=True`` changes nothing"""
    from step_amd.runner import native_runner
    ds = torch.utils.data.TensorDataset(torch.arange(12.0).view(6, 2), torch.arange(12.0).view(6, 2) * 0.5)
    plain = list(torch.utils.data.DataLoader(ds, batch_size=2))
    R = native_runner(_DummyBase, native_tail=True)
    r, base = R({}), _DummyBase({})
    assert r._tail_scaler() is None
    losses = [(float(r.train_iters(1, it, d)), float(base.train_iters(1, it, d))) for it, d in enumerate(plain)]
    assert all(a == b for a, b in losses)
    r.print_epoch_meters("train")
    base.print_epoch_meters("train")
    assert r.printed == base.printed and not r._pending


def test_work_buffer_size_needs_no_device():
    from step_amd import _lib
    n = _lib.lib().step_train_tail_work_doubles()
    assert isinstance(n, int) and n >= 12          # two halves of six sums


def test_bad_arguments_are_refused_on_the_host():
    from step_amd.step_loss import step_loss_native, train_tail
    x = torch.zeros(2, 12, 3, 1)
    t = torch.full((2, 4, 4), 0.5)
    with pytest.raises(ValueError):          # CPU tensors: there is no fall-back path
        train_tail(x, x, t, t, 1.0, horizons=3)
    with pytest.raises(ValueError):
        step_loss_native(x, x, t, t, torch.ones(()), horizons=3)          # a device-resident coefficient belongs to the graph-captured step
