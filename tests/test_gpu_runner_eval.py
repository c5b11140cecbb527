"""The runner's validation and test passes on the device: ``native_runner(..., native_eval=True)`` (validation meters from one
``EvalMetrics`` per pass) and ``eval_batch_size`` (coalesced origin batches) around the step_small model of tests/test_gpu_eval_cache.py,
``EvalMetrics.update(group=)``, and ``TSFormerRunner.test`` under ``native_pretrain``.  Host side: tests/test_runner_eval_host.py.

Bounds.  Device meters against torch's f32 formulas on the same predictions: relative 1e-5, the bound of tests/test_gpu_eval_metrics.py
for the kernel against the reference's metrics (an f32 mean over 3 * 12 * 37 elements here, the kernel sums the same terms in f64).  Two
ways of accumulating the same elements, and a repeated pass over bit-identical predictions: relative 1e-12 (f64 sums of identical f32
terms).  ``pretrain_tail`` against the base path: 2e-5, the bound of test_runner_native_pretrain_equals_the_base_class_path."""
import pickle
import random

import numpy as np
import pytest
import torch

from tests.eval_runner_double import EvalRunnerDouble
from tests.runner_double import masked_mae
from tests.test_gpu_eval_cache import BATCHES, _bytes, _fresh, _reseed
from tests.test_gpu_eval_metrics import MEAN, STD, _torch_three
from tests.test_gpu_pretrain_tail import PretrainRunnerDouble, runner_problem

pytestmark = pytest.mark.gpu

NAMES = ("MAE", "RMSE", "MAPE")
ORIGINS = [t for b in BATCHES for t in b]


def _batches(loader, mask_sensor=False):
    """the three batches of 3 origins as (future, history, long history reference); ``mask_sensor``: sensor 0's labels rescale to 0.0"""
    out = []
    for t0 in BATCHES:
        hist, ref, fut = loader.batch(t0)
        if mask_sensor:
            fut = fut.clone()
            fut[:, :, 0, 0] = -MEAN / STD
        out.append((fut, hist, ref))
    return out


def _runner(model, cls=EvalRunnerDouble, val_loader=None, **switches):
    from step_amd.runner import native_runner
    cfg = {"model": model, "loss": masked_mae, "scaler": (MEAN, STD), "cl": None, "val_loader": val_loader}
    runner = native_runner(cls, **switches)(cfg)
    runner.val_data_loader = runner.build_val_data_loader(cfg)
    return runner


def _validate(runner, model):
    """one validate() from fresh seeds and fresh meters -> (val_ meter calls seen by the base class before the first flush, the pass's
    predictions, the meter averages)"""
    before = []
    flush = type(runner).flush_meters

    def spy():
        before.append([c for c in runner.meter_log if c[0].startswith("val_")])
        return flush(runner)

    runner.flush_meters = spy
    runner.reset_epoch_meters()
    del runner.meter_log[:], runner.predictions[:]
    _reseed(model)
    runner.validate(train_epoch=1)
    del runner.flush_meters
    return before[0], list(runner.predictions), {k: runner.meters["val_" + k].avg for k in NAMES}


def _expected(predictions, labels, null_val, slices=None):
    """mean over the batches of the three torch formulas on the rescaled tensors (f32, on the host)"""
    rows = []
    for p, y in zip(predictions, labels):
        p, y = p.cpu() * STD + MEAN, y.cpu() * STD + MEAN
        rows.append(_torch_three(p, y, null_val))
    return dict(zip(NAMES, np.mean(np.array(rows, dtype=np.float64), axis=0)))


def _assert_meters(got, want, rel, what):
    for k in NAMES:
        print(f"{what}: val_{k} = {got[k]!r}, expected {want[k]!r}, relative difference {abs(got[k] - want[k]) / abs(want[k]):.3e}")
    for k in NAMES:
        assert got[k] == pytest.approx(want[k], rel=rel), (what, k)


# ---------------------------------------------------------------------------------------------- 1: native against base, same batches
def test_native_eval_equals_the_base_path_on_the_same_batches():
    model, loader = _fresh("bf16")
    data = _batches(loader)
    base = _runner(model, native_eval=False)
    base.val_data_loader = data
    seen0, preds0, meters0 = _validate(base, model)
    assert base.val_base_calls == 3 and len(seen0) == 9 and base._val_metrics is None
    native = _runner(model, native_eval=True)
    native.val_data_loader = data
    seen1, preds1, meters1 = _validate(native, model)
    assert native.val_base_calls == 0
    assert seen1 == []                                            # no val_ meter was fed before the flush
    assert [(name, n) for name, _v, n in native.meter_log] == [("val_" + k, 3) for k in NAMES]          # one call per metric, n = batches
    assert len(preds1) == 3 and all(torch.equal(x, y) for x, y in zip(preds1, preds0))
    _assert_meters(meters1, meters0, 1e-5, "native_eval against the base path")
    assert native.val_mae_at_validating_end == meters1["MAE"]     # in place before save_best_model reads it
    # a second pass on the same runner: the accumulator was reset
    _seen, preds2, meters2 = _validate(native, model)
    assert all(torch.equal(x, y) for x, y in zip(preds2, preds1))
    assert [(name, n) for name, _v, n in native.meter_log] == [("val_" + k, 3) for k in NAMES]
    _assert_meters(meters2, meters1, 1e-12, "second validate()")


# ---------------------------------------------------------------------------------------------- 2: a masked sensor, a NaN null_val
@pytest.mark.parametrize("null_val", [0.0, float("nan")], ids=["zero", "nan"])
def test_masked_sensor_and_nan_null_val_against_the_torch_formulas(null_val):
    model, loader = _fresh("bf16")
    data = _batches(loader, mask_sensor=True)
    native = _runner(model, native_eval=True)
    native.null_val = null_val
    native.val_data_loader = data
    seen, preds, meters = _validate(native, model)
    assert native.val_base_calls == 0 and seen == []
    assert [(name, n) for name, _v, n in native.meter_log] == [("val_" + k, 3) for k in NAMES]
    labels = [fut[..., 0:1] for fut, _h, _r in data]
    rescaled = labels[0][:, :, 0, 0] * STD + MEAN
    assert float(rescaled.abs().max()) < 5e-5                     # the masked sensor is inside the reference's atol of 0.0
    want = _expected(preds, labels, null_val)
    _assert_meters(meters, want, 1e-5, f"null_val = {null_val}")
    unmasked = _expected(preds, labels, float("nan") if null_val == 0.0 else 0.0)
    assert abs(unmasked["MAE"] - want["MAE"]) > 1e-3 * want["MAE"]          # the mask does matter on this data


# ---------------------------------------------------------------------------------------------- 3: coalescing
def _dataset(tmp_path, loader):
    from step_amd.runner import DeviceForecastingDataset
    with open(tmp_path / "data.pkl", "wb") as f:
        pickle.dump({"processed_data": loader.data.cpu().numpy()}, f)
    with open(tmp_path / "index.pkl", "wb") as f:
        pickle.dump({k: [(t - 12, t, t + 12) for t in ORIGINS] for k in ("train", "valid", "test")}, f)
    return DeviceForecastingDataset(str(tmp_path / "data.pkl"), str(tmp_path / "index.pkl"), "valid", loader.long_len)


def test_coalesced_validation_pass(tmp_path):
    model, loader = _fresh("bf16")
    ds = _dataset(tmp_path, loader)
    series = loader.data[:, :, 0].cpu()
    label = torch.stack([series[t:t + 12] for t in ORIGINS]).unsqueeze(-1)          # [9, 12, N, 1], normalised
    model.tsformer._events = []

    def host_loader():
        return torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False)

    runner = _runner(model, val_loader=host_loader(), native_eval=True, eval_batch_size=4, eval_cache_bytes=_bytes(9))
    assert runner.val_data_loader.coalesce == 2 and runner.val_data_loader.group_size == 2 and len(runner.val_data_loader) == 3
    seen, preds, meters = _validate(runner, model)
    assert [p.shape[0] for p in preds] == [4, 4, 1] and runner.val_base_calls == 0 and seen == []
    assert [(name, n) for name, _v, n in runner.meter_log] == [("val_" + k, 5) for k in NAMES]
    every = torch.cat(preds).cpu()
    cuts = ((0, 2), (2, 4), (4, 6), (6, 8), (8, 9))
    want = _expected([every[a:b] for a, b in cuts], [label[a:b] for a, b in cuts], 0.0)
    _assert_meters(meters, want, 1e-5, "coalesced by 2, per loader batch")
    # with the evaluation cache, a second coalesced pass launches no encoder and predicts the same bits
    launches = len(model.tsformer._events)
    assert launches == 3 and model.eval_cache_stats["windows_stored"] == 9
    _seen, preds2, meters2 = _validate(runner, model)
    assert len(model.tsformer._events) == launches and model.eval_cache_stats["window_hits"] == 9
    assert [p.shape[0] for p in preds2] == [4, 4, 1] and all(torch.equal(x, y) for x, y in zip(preds2, preds))
    _assert_meters(meters2, meters, 1e-12, "second coalesced pass")
    # eval_batch_size=None: the loader's own five batches
    model.eval_cache_bytes = 0
    plain = _runner(model, val_loader=host_loader(), native_eval=True)
    assert plain.val_data_loader.coalesce == 1 and len(plain.val_data_loader) == 5
    _seen, preds5, meters5 = _validate(plain, model)
    assert [p.shape[0] for p in preds5] == [2, 2, 2, 2, 1]
    assert [(name, n) for name, _v, n in plain.meter_log] == [("val_" + k, 5) for k in NAMES]
    want5 = _expected(preds5, [label[a:b] for a, b in cuts], 0.0)
    _assert_meters(meters5, want5, 1e-5, "uncoalesced")


# ---------------------------------------------------------------------------------------------- 4: EvalMetrics.update(group=)
def test_update_in_groups_equals_separate_updates():
    from step_amd import EvalMetrics
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(5, 12, 37, 1, generator=gen).cuda()
    y = torch.randn(5, 12, 37, 3, generator=gen).cuda()
    y[1, :, 4, 0] = -MEAN / STD                                    # a masked sensor in one window
    y = y[..., 0:1]                                               # a strided view, as the runner's target selection gives
    apart = EvalMetrics(12, 0.0, rescale=(STD, MEAN))
    for a, b in ((0, 2), (2, 4), (4, 5)):
        apart.update(p[a:b], y[a:b])
    want = apart.result()
    grouped = EvalMetrics(12, 0.0, rescale=(STD, MEAN))
    grouped.update(p, y, group=2)
    got = grouped.result()
    assert got.batches == want.batches == 3
    for x, w, what in ((got.per_horizon, want.per_horizon, "per horizon"), (got.overall, want.overall, "overall"),
                       (got.batch_mean, want.batch_mean, "batch mean")):
        print(f"group=2, {what}: largest relative difference {float(np.max(np.abs(x - w) / np.abs(w))):.3e}")
        assert np.allclose(x, w, rtol=1e-12, atol=0.0)
    whole = EvalMetrics(12, 0.0, rescale=(STD, MEAN))
    whole.update(p, y)
    one = whole.result()
    for g in (None, 5, 8):                                        # one launch over everything, as without the keyword
        m = EvalMetrics(12, 0.0, rescale=(STD, MEAN))
        m.update(p, y, group=g)
        r = m.result()
        assert r.batches == 1 and np.array_equal(r.per_horizon, one.per_horizon) and np.array_equal(r.batch_mean, one.batch_mean)
    assert not np.allclose(one.batch_mean, want.batch_mean, rtol=1e-6, atol=0.0)          # the grouping does change the batch mean
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="group"):
            grouped.update(p, y, group=bad)
    after = grouped.result()
    assert after.batches == 3 and np.array_equal(after.overall, got.overall)          # refused before anything was launched


# ---------------------------------------------------------------------------------------------- 5: the forward's outputs do not qualify
class _DoublePrecisionForward(EvalRunnerDouble):
    def forward(self, data, epoch=None, iter_num=None, train=True, **kwargs):
        out = super().forward(data, epoch=epoch, iter_num=iter_num, train=train, **kwargs)
        return (out[0].double(),) + tuple(out[1:])


def test_fallback_after_the_forward_gives_the_base_tail():
    model, loader = _fresh("bf16")
    data = _batches(loader)
    base = _runner(model, cls=_DoublePrecisionForward, native_eval=False)
    base.val_data_loader = data
    _seen, _preds, meters0 = _validate(base, model)
    native = _runner(model, cls=_DoublePrecisionForward, native_eval=True)
    native.val_data_loader = data
    seen, _preds, meters1 = _validate(native, model)
    assert base.val_base_calls == 3 and native.val_base_calls == 0          # the branch was taken, and fell back after the forward
    assert len(seen) == 9 and all(n == 1 for _name, _v, n in seen)          # the base tail's per-batch calls
    assert native._val_metrics is None
    _assert_meters(meters1, meters0, 1e-12, "float64 prediction: the same torch ops as the base tail")


# ---------------------------------------------------------------------------------------------- 6: TSFormerRunner.test
class PretrainTestRunnerDouble(PretrainRunnerDouble):
    """adds ``TSFormerRunner.test`` (step/step_runner/tsformer_runner.py:73-90) restated, and a log of the meter calls"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.test_base_calls = 0
        self.meter_log = []

    def update_epoch_meter(self, name, value, n=1):
        self.meter_log.append((name, float(value), n))
        super().update_epoch_meter(name, value, n)

    @torch.no_grad()
    def test(self):
        self.test_base_calls += 1
        for _, data in enumerate(self.test_data_loader):
            forward_return = self.forward(data=data, epoch=None, iter_num=None, train=False)
            mean, std = self.scaler["args"]["mean"], self.scaler["args"]["std"]
            prediction_rescaled, real_value_rescaled = forward_return[0] * std + mean, forward_return[1] * std + mean
            for metric_name, metric_func in self.metrics.items():
                metric_item = metric_func(prediction_rescaled, real_value_rescaled, null_val=self.null_val)
                self.update_epoch_meter("test_" + metric_name, metric_item.item())


class _SeededBatches:
    """hands out the batches with ``random`` seeded per batch: the same masks on both sides, as ``iterations()`` does"""

    def __init__(self, data):
        self.data = data

    def __iter__(self):
        for it, batch in enumerate(self.data):
            random.seed(1234 + it)
            yield batch


def _test_pass(native_pretrain, loss_fn=masked_mae):
    from step_amd.runner import native_runner
    model, data = runner_problem()
    runner = native_runner(PretrainTestRunnerDouble, native_pretrain=native_pretrain)(
        {"model": model, "loss": loss_fn, "scaler": (200.0, 150.0), "cl": None})
    runner.test_data_loader = _SeededBatches(data)
    runner.test()
    before = list(runner.meter_log)
    pending = {k: len(v) for k, v in runner._pending.items()}
    runner.print_epoch_meters("test")
    return runner, before, pending, {k: runner.meters["test_" + k].avg for k in NAMES}


def test_tsformer_runner_test_under_native_pretrain():
    base, before0, pending0, meters0 = _test_pass(False)
    assert base.test_base_calls == 1 and len(before0) == 6 and pending0 == {}
    native, before1, pending1, meters1 = _test_pass(True)
    assert native.test_base_calls == 0
    assert before1 == [] and pending1 == {"test_" + k: 2 for k in NAMES}          # nothing was read back per batch
    assert all(native.meters["test_" + k].n == 2 and base.meters["test_" + k].n == 2 for k in NAMES)
    for k in NAMES:
        print(f"test_{k}: native {meters1[k]!r}, base {meters0[k]!r}")
    for k in NAMES:
        assert meters1[k] == pytest.approx(meters0[k], rel=2e-5), k
    per_batch = [v for name, v, _n in before0 if name == "test_MAE"]
    assert per_batch[0] != per_batch[1]                           # two different batches went in


def test_tsformer_runner_test_keeps_the_base_path_for_another_loss():
    def my_loss(*args, **kwargs):
        return masked_mae(*args, **kwargs)
    base, _b, _p, meters0 = _test_pass(False, loss_fn=my_loss)
    native, before, pending, meters1 = _test_pass(True, loss_fn=my_loss)
    assert native.test_base_calls == 1 and len(before) == 6 and pending == {}
    for k in NAMES:
        assert meters1[k] == pytest.approx(meters0[k], rel=2e-5), k
