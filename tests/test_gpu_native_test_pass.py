"""``native_runner(..., native_test=True)`` on one rank: the forecasting ``test()`` from one ``EvalMetrics`` -- one launch per batch, nothing
concatenated, one read-back -- against the base class's ``test()`` (tests/spread_double.py: ``base_tsf_runner.py:277-318`` restated) on
the same predictions, around the step_small model of tests/test_gpu_eval_cache.py.

Bound: relative 1e-5, the bound of tests/test_gpu_eval_metrics.py for the kernel against the reference's metrics (float32 torch formulas
against f64 sums of the same float32 terms).  The logged lines carry four decimals: two numbers within ``d`` of each other print within
``d + 1e-4`` (each is rounded by at most 0.5e-4), which is what the parsed lines are held to; the table itself is held to 1e-5."""
import re

import numpy as np
import pytest
import torch

from tests.runner_double import masked_mae
from tests.spread_double import TestPassDouble
from tests.test_gpu_eval_cache import _fresh, _reseed
from tests.test_gpu_eval_metrics import MEAN, STD
from tests.test_gpu_runner_eval import NAMES, _batches

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^Evaluate best model on test data for horizon (\d+), Test MAE: (\d+\.\d{4}), Test RMSE: (\d+\.\d{4}), Test MAPE: (\d+\.\d{4})$")


class _Readbacks:
    """counts ``.item()`` / ``.cpu()`` / ``.tolist()`` on device tensors while active: each makes the host wait for the stream"""

    def __enter__(self):
        self.count, self._saved = 0, {}
        for name in ("item", "cpu", "tolist"):
            original = self._saved[name] = getattr(torch.Tensor, name)

            def counted(t, *args, _original=original, **kwargs):
                if t.is_cuda:
                    self.count += 1
                return _original(t, *args, **kwargs)
            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, saved in self._saved.items():
            setattr(torch.Tensor, name, saved)


def _runner(model, data, **switches):
    from step_amd.runner import native_runner
    runner = native_runner(TestPassDouble, **switches)({"model": model, "loss": masked_mae, "scaler": (MEAN, STD), "cl": None})
    runner.test_data_loader = data
    return runner


def _test_pass(runner, model):
    runner.reset_epoch_meters()
    del runner.meter_log[:], runner.predictions[:], runner.logger.lines[:]
    _reseed(model)
    model.eval()
    with _Readbacks() as rb:
        runner.test()
    lines = [LINE.match(line) for line in runner.logger.lines]
    assert all(m is not None for m in lines), runner.logger.lines
    table = np.array([[float(x) for x in m.groups()[1:]] for m in lines])
    assert [int(m.group(1)) for m in lines] == list(range(1, 13))
    return {k: runner.meters["test_" + k].avg for k in NAMES}, table, list(runner.predictions), rb.count


def test_native_test_equals_the_base_test_on_the_same_predictions(monkeypatch):
    from step_amd import EvalMetrics
    model, loader = _fresh("bf16")
    data = _batches(loader, mask_sensor=True)
    base = _runner(model, data, native_test=False)
    meters0, lines0, preds0, readbacks0 = _test_pass(base, model)
    assert base.test_base_calls == 1 and readbacks0 >= 12 * 3 + 3          # the base pass reads every number back by itself
    tables, updates = [], []
    result, update = EvalMetrics.result, EvalMetrics.update
    monkeypatch.setattr(EvalMetrics, "result", lambda self, *a, **k: tables.append(result(self, *a, **k)) or tables[-1])
    monkeypatch.setattr(EvalMetrics, "update", lambda self, p, r, **k: updates.append(tuple(p.shape)) or update(self, p, r, **k))
    native = _runner(model, data, native_test=True)
    meters1, lines1, preds1, readbacks1 = _test_pass(native, model)
    assert native.test_base_calls == 0 and native.eval_readbacks == 1
    assert readbacks1 == 1 and len(tables) == 1                            # ONE read-back for the whole pass
    assert updates == [(3, 12, 37, 1)] * 3                                 # one launch per batch, nothing concatenated
    assert len(preds1) == 3 and all(torch.equal(x, y) for x, y in zip(preds1, preds0))
    assert [(name, n) for name, _v, n in native.meter_log] == [("test_" + k, 1) for k in NAMES]
    for k in NAMES:
        print(f"test_{k}: native {meters1[k]!r}, base {meters0[k]!r}, relative difference {abs(meters1[k] - meters0[k]) / abs(meters0[k]):.3e}")
    for k in NAMES:
        assert meters1[k] == pytest.approx(meters0[k], rel=1e-5), k
    # the twelve per-horizon triples: the table against the torch formulas on the same (rescaled) predictions, the lines against the base's
    res = tables[0]
    every = torch.cat(preds0).cpu() * STD + MEAN
    label = torch.cat([fut[..., 0:1] for fut, _h, _r in data]).cpu() * STD + MEAN
    from tests.test_gpu_eval_metrics import _torch_three
    want = np.array([_torch_three(every[:, h], label[:, h], 0.0) for h in range(12)], dtype=np.float64)
    rel = np.abs(res.per_horizon - want) / np.abs(want)
    print(f"per-horizon table against the torch formulas: largest relative difference {float(rel.max()):.3e}")
    assert float(rel.max()) <= 1e-5
    assert np.all(np.abs(lines1 - lines0) <= 1e-5 * np.abs(lines0) + 1e-4), (lines1, lines0)
    assert np.all(np.abs(lines1 - res.per_horizon) <= 0.5e-4 + 1e-9)       # the lines print the table
    assert len(set(map(tuple, lines0.tolist()))) == 12                     # twelve different horizons went in
    # a second pass on the same runner starts from a fresh accumulator
    meters2, lines2, _p, readbacks2 = _test_pass(native, model)
    assert readbacks2 == 1 and np.array_equal(lines2, lines1) and all(meters2[k] == pytest.approx(meters1[k], rel=1e-12) for k in NAMES)


def test_only_the_evaluation_horizons_are_logged():
    model, loader = _fresh("bf16")
    native = _runner(model, _batches(loader), native_test=True)
    native.evaluation_horizons = [2, 11]
    native.reset_epoch_meters()
    _reseed(model)
    native.test()
    assert [int(LINE.match(line).group(1)) for line in native.logger.lines] == [3, 12]


def _custom_metric(preds, labels, null_val=0.0):
    return masked_mae(preds, labels, null_val=null_val)


@pytest.mark.parametrize("broken", ["metric", "scaler", "switch_off"])
def test_the_base_test_runs_when_a_condition_fails(broken):
    model, loader = _fresh("bf16")
    runner = _runner(model, _batches(loader), native_test=broken != "switch_off")
    if broken == "metric":
        runner.metrics = {"MAE": _custom_metric, "RMSE": runner.metrics["RMSE"], "MAPE": runner.metrics["MAPE"]}          # not basicts'
    if broken == "scaler":
        runner.scaler = {"func": "re_standard_transform", "args": {"mean": torch.tensor(MEAN), "std": torch.tensor(STD)}}      # not scalars
    meters, lines, preds, readbacks = _test_pass(runner, model)
    assert runner.test_base_calls == 1 and runner.eval_readbacks == 0 and readbacks >= 39 and len(preds) == 3
    assert all(np.isfinite(v) for v in meters.values()) and lines.shape == (12, 3)


def test_native_test_works_without_native_eval_and_leaves_validation_alone():
    model, loader = _fresh("bf16")
    runner = _runner(model, _batches(loader), native_test=True, native_eval=False)
    assert runner._eval_scaler() is None and runner._eval_conditions() == (MEAN, STD)
