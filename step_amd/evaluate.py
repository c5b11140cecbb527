"""Device-side validation / test pass: the reference's masked MAE / RMSE / MAPE per horizon, over the whole pass and as the mean of the
per-batch values, accumulated by ``libstep_hip`` (``csrc/eval_metrics.hip``) while the pass runs and read back ONCE.

The reference's test pass (``basicts/runners/base_tsf_runner.py:277-318``) keeps every prediction, rescales the concatenation and slices
it per horizon for ``basicts/metrics/{mae,rmse,mape}.py``; its validation pass (``:257-273``) averages the per-batch values and reads
three numbers back per batch.  ``EvalMetrics`` gives both tables from one launch per batch:

    m = EvalMetrics(horizons=12, null_val=0.0, rescale=(std, mean))
    for ...:
        m.update(prediction, future[..., 0])        # queued; nothing is copied, nothing is read back
    r = m.result()                                  # r.per_horizon [H, 3], r.overall [3], r.batch_mean [3], r.batches

``STEP.evaluate(loader, origins, ...)`` (``evaluate_pass`` below) is that loop over a device-resident series.  In eval mode every window
is independent of its batch (BatchNorm uses its running statistics, nothing needs a gradient), so ``batch_size`` may be much larger than
the training configuration's: the host work of a forward is then shared by more windows.
"""
import ctypes
import math
import numbers
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

METRICS = ("MAE", "RMSE", "MAPE")          # the columns of every table below
MAX_HORIZONS = 64


@dataclass
class EvalResult:
    """``per_horizon`` float64 [len(horizons), 3] (columns ``METRICS``), ``overall`` [3] over all horizons and windows, ``batch_mean``
    [3]: the equal-weight mean over the ``batches`` updates of each update's own overall metrics (the validation meters' average)."""
    per_horizon: np.ndarray
    overall: np.ndarray
    batch_mean: np.ndarray
    batches: int
    horizons: tuple


def _view3(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise ValueError(f"EvalMetrics.update: {what} must be an f32 cuda tensor")
    if t.dim() == 4 and t.shape[3] == 1:
        t = t[..., 0]
    if t.dim() != 3:
        raise ValueError(f"EvalMetrics.update: {what} must be [B, H, N] or [B, H, N, 1], got {tuple(t.shape)}")
    return t


def _strides(t, what):
    out = []
    for size, stride in zip(t.shape, t.stride()):
        if size > 1 and stride < 1:
            raise ValueError(f"EvalMetrics.update: {what} has a non-positive stride {t.stride()} (an expanded view?)")
        out.append(max(int(stride), 1))          # the stride of a dimension of one element is never used
    return out


class EvalMetrics:
    """Accumulator of one pass.  ``rescale = (scale, shift)``: the metrics are taken on ``x * scale + shift`` of both tensors (the
    scaler's std and mean; ``None``: the tensors as they are).  ``null_val`` may be NaN (the reference's default: only NaN labels
    are masked).  Updates of one accumulator must be queued on one stream."""

    def __init__(self, horizons=12, null_val=0.0, rescale=None, device=None):
        self.horizons = int(horizons)
        n = _lib.lib().step_eval_metrics_acc_doubles(self.horizons)
        if n <= 0:
            raise ValueError(f"EvalMetrics: horizons = {horizons} is not in 1..{MAX_HORIZONS}")
        self.null_val = float(null_val)
        self.scale, self.shift = (1.0, 0.0) if rescale is None else (float(rescale[0]), float(rescale[1]))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("EvalMetrics accumulates on an AMD GPU: libstep_hip has no CPU fallback")
        self._acc = torch.zeros(n, dtype=torch.float64, device=dev)
        self._out = torch.empty((self.horizons + 2) * 3, dtype=torch.float64, device=dev)
        self.batches = 0

    def reset(self):
        self._acc.zero_()
        self.batches = 0

    def update(self, pred, real, group=None):
        """one accumulate launch over the whole of ``pred`` / ``real``; with ``group = g`` one launch per ``g`` consecutive windows
        (views of the two tensors, nothing is copied; the last group may be short), so that ``batches`` and ``batch_mean`` are what
        separate updates of ``g`` windows each would have given: a loader that coalesces ``k`` batches of ``g`` windows into one
        forward keeps the validation meters' per-loader-batch average"""
        if group is not None:
            if isinstance(group, bool) or not isinstance(group, numbers.Integral) or group < 1:
                raise ValueError(f"EvalMetrics.update: group = {group!r} must be a positive integer (or None)")
            group = int(group)
        p, r = _view3(pred, "pred"), _view3(real, "real")
        if p.shape != r.shape or p.shape[1] != self.horizons or 0 in p.shape:
            raise ValueError(f"EvalMetrics.update: pred {tuple(pred.shape)} and real {tuple(real.shape)} must be one non-empty "
                             f"[B, {self.horizons}, N] shape")
        if p.device != self._acc.device or r.device != self._acc.device:
            raise ValueError(f"EvalMetrics.update: tensors on {p.device} / {r.device}, accumulator on {self._acc.device}")
        B, H, N = p.shape
        ps, rs = _strides(p, "pred"), _strides(r, "real")          # (checked on the whole tensors: refused before anything is launched)
        g = B if group is None else min(group, B)
        for at in range(0, B, g):
            n = min(g, B - at)
            _lib.call("step_eval_metrics_accumulate", ctypes.c_void_p(p.data_ptr() + 4 * at * ps[0]), *ps,
                      ctypes.c_void_p(r.data_ptr() + 4 * at * rs[0]), *rs, n, H, N, self.scale, self.shift, self.null_val,
                      _lib.ptr(self._acc), _lib.stream())
            self.batches += 1

    def result(self, horizons=None):
        """the single device-to-host copy of the pass; the accumulator stays as it is (more updates may follow)"""
        H = self.horizons
        rows = tuple(range(H)) if horizons is None else tuple(int(h) for h in horizons)
        if any(not 0 <= h < H for h in rows):
            raise ValueError(f"EvalMetrics.result: horizons {rows} not all in 0..{H - 1}")
        _lib.call("step_eval_metrics_finish", _lib.ptr(self._acc), H, _lib.ptr(self._out), _lib.stream())
        table = self._out.cpu().numpy().reshape(H + 2, 3)
        return EvalResult(per_horizon=table[list(rows)].copy(), overall=table[H].copy(), batch_mean=table[H + 1].copy(),
                          batches=self.batches, horizons=rows)


def _scale_shift(scaler):
    """(std, mean) of the scaler: ``None``, a ``(mean, std)`` pair, ``{"mean": .., "std": ..}`` or the reference's
    ``{"func": .., "args": {"mean": .., "std": ..}}`` (``base_tsf_runner.py:238``)"""
    if scaler is None:
        return None
    if isinstance(scaler, dict):
        args = scaler.get("args", scaler)
        mean, std = args["mean"], args["std"]
    else:
        mean, std = scaler
    mean, std = float(mean), float(std)
    if not (math.isfinite(mean) and math.isfinite(std)):
        raise ValueError(f"STEP.evaluate: scaler mean = {mean}, std = {std} must be finite")
    return std, mean


def evaluate_pass(model, loader, origins=None, scaler=None, null_val=0.0, batch_size=None, target_channel=0, horizons=None,
                  return_predictions=False):
    """``STEP.evaluate``: one validation / test pass of ``model`` over the windows at ``origins`` (host integers, walked in order in chunks
    of ``batch_size``, default 8).  ``loader``: a ``DeviceWindowLoader``, or a ``DeviceForecastingDataset`` (``origins`` then defaults to
    its index).  Every chunk is one forward in eval mode under ``torch.no_grad()`` followed by one ``EvalMetrics.update`` against channel
    ``target_channel`` of the future window; nothing is read back before the table.  ``scaler``: see ``_scale_shift``.  ``horizons``: the rows
    reported (the reference's ``EVALUATION_HORIZONS``; default all).  Returns an ``EvalResult``, with ``return_predictions=True`` the
    pair ``(EvalResult, normalised predictions [W, H, N] on the device)``.  The ``training`` flag is restored on exit."""
    from .step_arch.step import DeviceWindowLoader
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("step_amd.STEP runs only on an AMD GPU: libstep_hip has no CPU fallback")
    if not isinstance(loader, DeviceWindowLoader):
        if not getattr(loader, "index_only", False):
            raise ValueError("STEP.evaluate: loader must be a DeviceWindowLoader or a DeviceForecastingDataset")
        if origins is None:
            origins = [idx[1] for idx in loader.index]
        loader = loader.device_loader(dev)
    if origins is None:
        raise ValueError("STEP.evaluate: a DeviceWindowLoader needs the forecast origins of the pass")
    if torch.is_tensor(origins) and origins.is_cuda:
        raise ValueError("STEP.evaluate: origins must be host integers (the evaluation cache keys on them without reading the device)")
    origins = [int(t) for t in origins]
    step = 8 if batch_size is None else int(batch_size)
    if step < 1 or not origins:
        raise ValueError(f"STEP.evaluate: batch_size = {batch_size} with {len(origins)} origins")
    H, N = loader.horizon, loader.data.shape[1]
    metrics = EvalMetrics(H, null_val, _scale_shift(scaler), device=dev)
    kept = torch.empty(len(origins), H, N, device=dev) if return_predictions else None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for at in range(0, len(origins), step):
                hist, ref, fut = loader.batch(origins[at:at + step])
                pred = model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=None, epoch=None)[0]
                metrics.update(pred, fut[..., int(target_channel)])
                if kept is not None:
                    kept[at:at + pred.shape[0]].copy_(pred[..., 0])
    finally:
        model.train(was_training)
    res = metrics.result(horizons)
    return (res, kept) if return_predictions else res
