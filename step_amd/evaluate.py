"""Device-side validation / test pass: the reference's masked MAE / RMSE / MAPE per horizon, over the whole pass and as the mean of the
per-batch values, accumulated by ``libstep_hip`` (``csrc/eval_metrics.hip``) while the pass runs and read back ONCE.

The reference's test pass (``basicts/runners/base_tsf_runner.py:277-318``) keeps every prediction, rescales the concatenation and slices
it per horizon for ``basicts/metrics/{mae,rmse,mape}.py``; its validation pass (``:257-273``) averages the per-batch values and reads
three numbers back per batch.  ``EvalMetrics`` gives both tables from one launch per batch:

    m = EvalMetrics(horizons=12, null_val=0.0, rescale=(std, mean))
    for ...:
        m.update(prediction, future[..., 0])        # queued; nothing is copied, nothing is read back
    r = m.result()                                  # r.per_horizon [H, 3], r.overall [3], r.batch_mean [3], r.batches

``EvalMetrics(..., nodes=N)`` keeps the same sums per sensor as well (``csrc/eval_nodes.hip``: a second launch per batch on the same
views, no atomics): ``r.per_node`` [N, H, 3] and ``r.per_node_overall`` [N, 3] come back in the same single copy, and
``update(..., out=)`` stores the rescaled prediction -- the value the metrics are taken on -- from that launch.

``STEP.evaluate(loader, origins, ...)`` (``evaluate_pass`` below) is that loop over a device-resident series.  In eval mode every window
is independent of its batch (BatchNorm uses its running statistics, nothing needs a gradient), so ``batch_size`` may be much larger than
the training configuration's: the host work of a forward is then shared by more windows.  The one thing that ties a window to its batch
is the graph learner's eval-mode sampling under ``STEP.eval_noise = "position"``; with ``"window"`` a pass is a function of the weights
and the windows alone, and ``evaluate_pass(..., process_group=)`` / ``EvalMetrics.all_reduce`` spread it over ranks.
"""
import ctypes
import math
import numbers
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .step_loss import _is_scalar, node_scaler

METRICS = ("MAE", "RMSE", "MAPE")          # the columns of every table below
MAX_HORIZONS = 64


@dataclass
class EvalResult:
    """``per_horizon`` float64 [len(horizons), 3] (columns ``METRICS``), ``overall`` [3] over all horizons and windows, ``batch_mean``
    [3]: the equal-weight mean over the ``batches`` updates of each update's own overall metrics (the validation meters' average).
    Of an accumulator with ``nodes=N``: ``per_node`` float64 [N, len(horizons), 3], the same three metrics of every sensor at the
    reported horizons, and ``per_node_overall`` [N, 3], over all horizons and windows (a sensor without a counted label: 0);
    otherwise both are ``None``."""
    per_horizon: np.ndarray
    overall: np.ndarray
    batch_mean: np.ndarray
    batches: int
    horizons: tuple
    per_node: np.ndarray = None
    per_node_overall: np.ndarray = None


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
    scaler's std and mean; ``None``: the tensors as they are).  Each of the two may be a scalar or N values (a per-node scaler, as
    ``step_amd.step_loss.node_scaler`` takes them: element ``(b, h, n)`` is then taken on ``x * scale[n] + shift[n]``; a length other
    than the tensors' N raises ``ValueError`` in ``update``).  ``null_val`` may be NaN (the reference's default: only NaN labels
    are masked).  Updates of one accumulator must be queued on one stream.

    ``nodes=N``: the five sums are also kept per (horizon, sensor) for tensors of N sensors, in a table f64 [5, H, N] that follows the
    accumulator in the SAME allocation (``reset`` and ``all_reduce`` cover both); every ``update`` then issues a second launch
    (``step_eval_node_metrics_accumulate``) over the same views, and ``result`` fills ``per_node`` / ``per_node_overall``."""

    def __init__(self, horizons=12, null_val=0.0, rescale=None, device=None, nodes=None):
        self.horizons = int(horizons)
        n = _lib.lib().step_eval_metrics_acc_doubles(self.horizons)
        if n <= 0:
            raise ValueError(f"EvalMetrics: horizons = {horizons} is not in 1..{MAX_HORIZONS}")
        self.nodes, table = None, 0
        if nodes is not None:
            if isinstance(nodes, bool) or not isinstance(nodes, numbers.Integral) or nodes < 1:
                raise ValueError(f"EvalMetrics: nodes = {nodes!r} must be a positive integer (or None)")
            self.nodes = int(nodes)
            table = _lib.lib().step_eval_node_table_doubles(self.horizons, self.nodes)
        self.null_val = float(null_val)
        self._nodes = None          # (scale, shift) of a per-node scaler as given; their device copies are node_scaler's
        if rescale is not None and not (_is_scalar(rescale[0]) and _is_scalar(rescale[1])):
            self._nodes = (rescale[0], rescale[1])
            self.scale = self.shift = None
        else:
            self.scale, self.shift = (1.0, 0.0) if rescale is None else (float(rescale[0]), float(rescale[1]))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("EvalMetrics accumulates on an AMD GPU: libstep_hip has no CPU fallback")
        # one allocation: the accumulator, then the per-node table (zeroed, reduced over ranks together); likewise what result() copies
        self._buf = torch.zeros(n + table, dtype=torch.float64, device=dev)
        self._acc, self._table = self._buf[:n], (self._buf[n:] if table else None)
        rows = (self.horizons + 2) * 3
        self._outbuf = torch.empty(rows + (self.horizons + 1) * (self.nodes or 0) * 3, dtype=torch.float64, device=dev)
        self._out, self._node_out = self._outbuf[:rows], (self._outbuf[rows:] if table else None)
        self.batches = 0
        self._reduced = False          # all_reduce ran since the last reset: the count of updates is the device's

    def reset(self):
        self._buf.zero_()
        self.batches = 0
        self._reduced = False

    def update(self, pred, real, group=None, out=None):
        """one accumulate launch over the whole of ``pred`` / ``real``; with ``group = g`` one launch per ``g`` consecutive windows
        (views of the two tensors, nothing is copied; the last group may be short), so that ``batches`` and ``batch_mean`` are what
        separate updates of ``g`` windows each would have given: a loader that coalesces ``k`` batches of ``g`` windows into one
        forward keeps the validation meters' per-loader-batch average.  With ``nodes`` the per-node launch follows each of them over
        the same views.  ``out`` (needs ``nodes``): a contiguous f32 ``[B, H, N]`` tensor on the accumulator's device that receives
        ``pred * scale + shift``, the value the metrics are taken on, stored by the per-node launch"""
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
        if self.nodes is not None and N != self.nodes:
            raise ValueError(f"EvalMetrics.update: tensors of {N} nodes, the accumulator was built with nodes = {self.nodes}")
        if out is not None:
            if self.nodes is None:
                raise ValueError("EvalMetrics.update: out= needs an accumulator built with nodes=N (the per-node launch stores it)")
            if not (torch.is_tensor(out) and out.dtype == torch.float32 and out.device == self._acc.device and out.is_contiguous()
                    and tuple(out.shape) == (B, H, N)):
                raise ValueError(f"EvalMetrics.update: out must be a contiguous f32 [{B}, {H}, {N}] tensor on {self._acc.device}")
        ps, rs = _strides(p, "pred"), _strides(r, "real")          # (checked on the whole tensors: refused before anything is launched)
        if self._nodes is None:
            entry, scaler, form = "step_eval_metrics_accumulate", (self.scale, self.shift), ""
        else:
            scale, shift = node_scaler(self._nodes[1], self._nodes[0], N, self._acc.device, "EvalMetrics.update")
            entry, scaler, form = "step_eval_metrics_accumulate_nodes", (_lib.ptr(scale), _lib.ptr(shift)), "_nodes"
        g = B if group is None else min(group, B)
        for at in range(0, B, g):
            n = min(g, B - at)
            _lib.call(entry, ctypes.c_void_p(p.data_ptr() + 4 * at * ps[0]), *ps, ctypes.c_void_p(r.data_ptr() + 4 * at * rs[0]), *rs,
                      n, H, N, *scaler, self.null_val, _lib.ptr(self._acc), _lib.stream())
            if self.nodes is not None:
                to = None if out is None else ctypes.c_void_p(out.data_ptr() + 4 * at * H * N)
                _lib.call("step_eval_node_metrics_accumulate" + form, ctypes.c_void_p(p.data_ptr() + 4 * at * ps[0]), *ps,
                          ctypes.c_void_p(r.data_ptr() + 4 * at * rs[0]), *rs, n, H, N, *scaler, self.null_val, _lib.ptr(self._table), to,
                          _lib.stream())
            self.batches += 1

    def result(self, horizons=None):
        """the single device-to-host copy of the pass; the accumulator stays as it is (more updates may follow)"""
        H = self.horizons
        rows = tuple(range(H)) if horizons is None else tuple(int(h) for h in horizons)
        if any(not 0 <= h < H for h in rows):
            raise ValueError(f"EvalMetrics.result: horizons {rows} not all in 0..{H - 1}")
        _lib.call("step_eval_metrics_finish", _lib.ptr(self._acc), H, _lib.ptr(self._out), _lib.stream())
        if self.nodes is not None:
            _lib.call("step_eval_node_metrics_finish", _lib.ptr(self._table), H, self.nodes, _lib.ptr(self._node_out), _lib.stream())
        # after all_reduce the accumulator's count of updates (slot 5H + 8, summed over the ranks) comes back with the table, in the one copy
        out = torch.cat([self._outbuf, self._acc[5 * H + 8:5 * H + 9]]) if self._reduced else self._outbuf
        flat = out.cpu().numpy()
        if self._reduced:
            self.batches = int(round(flat[-1]))
        table = flat[:(H + 2) * 3].reshape(H + 2, 3)
        per_node = per_node_overall = None
        if self.nodes is not None:
            nodes = flat[(H + 2) * 3:(H + 2) * 3 + (H + 1) * self.nodes * 3].reshape(H + 1, self.nodes, 3)          # [H + 1, N, 3] as finished
            per_node, per_node_overall = np.ascontiguousarray(nodes[list(rows)].transpose(1, 0, 2)), nodes[H].copy()
        return EvalResult(per_horizon=table[list(rows)].copy(), overall=table[H].copy(), batch_mean=table[H + 1].copy(),
                          batches=self.batches, horizons=rows, per_node=per_node, per_node_overall=per_node_overall)

    def all_reduce(self, process_group=None):
        """Merge the accumulators of the ranks of ``process_group`` (None: the default group): ONE SUM all-reduce of the f64
        allocation (the accumulator and, with ``nodes``, the per-node table behind it) through ``torch.distributed``, in place on the device, nothing read back.  Every rank calls it once, between its
        last ``update`` and ``result``; afterwards every rank holds the pass of all ranks' updates together, and ``batches`` is the sum
        over the ranks from the next ``result()`` on (it is the accumulator's own count of updates and comes back with the table).

        Why a plain sum is the merge (accumulator layout of ``csrc/eval_metrics.hip``, H horizons): slots ``[0, 5H)`` are the five sums
        (|err|, err^2, count, APE, its count) per horizon over all updates, ``[5H+5, 5H+8)`` the sum over updates of each update's own
        MAE / RMSE / MAPE and ``5H+8`` the number of updates -- all sums of per-update terms, so the sum over ranks is what one
        accumulator fed every update would hold, up to the order of the f64 additions.  The per-call slots ``[5H, 5H+5)`` and the ticket
        ``5H+9`` are zero between calls on every rank, and 0 + 0 = 0 keeps them so.  ``result`` then divides as always.  A rank
        without any update contributes zeros.  The per-node table (``csrc/eval_nodes.hip``: the same five sums per (horizon, node)
        over all updates) is a sum of per-update terms like the first 5H slots, so the same argument holds for it; every rank must
        have been built with the same ``nodes`` (the ranks reduce the same number of doubles)."""
        import torch.distributed as dist
        dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=process_group)
        self._reduced = True


def _scale_shift(scaler):
    """(std, mean) of the scaler: ``None``, a ``(mean, std)`` pair, ``{"mean": .., "std": ..}`` or the reference's
    ``{"func": .., "args": {"mean": .., "std": ..}}`` (``base_tsf_runner.py:238``).  Scalars come back as floats; N values (numpy
    arrays or tensors, the per-node scaler of ``--norm_each_channel``) as they are, for ``EvalMetrics`` to check against the data"""
    if scaler is None:
        return None
    if isinstance(scaler, dict):
        args = scaler.get("args", scaler)
        mean, std = args["mean"], args["std"]
    else:
        mean, std = scaler
    if not (_is_scalar(mean) and _is_scalar(std)):
        return std, mean          # (node_scaler checks length and finiteness where N is known: in front of the first update's launch)
    mean, std = float(mean), float(std)
    if not (math.isfinite(mean) and math.isfinite(std)):
        raise ValueError(f"STEP.evaluate: scaler mean = {mean}, std = {std} must be finite")
    return std, mean


def eval_rank_chunks(n_chunks, rank, world):
    """The chunks (batches) of an evaluation pass that ``rank`` of ``world`` evaluates when the pass is spread over the ranks: chunk
    ``c`` belongs to rank ``c % world``.  Every chunk keeps the composition it has in a single-process pass; only who runs it changes."""
    n_chunks, rank, world = int(n_chunks), int(rank), int(world)
    if world < 1 or not 0 <= rank < world or n_chunks < 0:
        raise ValueError(f"eval_rank_chunks: n_chunks = {n_chunks}, rank = {rank}, world = {world}")
    return list(range(rank, n_chunks, world))


def evaluate_pass(model, loader, origins=None, scaler=None, null_val=0.0, batch_size=None, target_channel=0, horizons=None,
                  return_predictions=False, process_group=None, per_node=False):
    """``STEP.evaluate``: one validation / test pass of ``model`` over the windows at ``origins`` (host integers, walked in order in chunks
    of ``batch_size``, default 8).  ``loader``: a ``DeviceWindowLoader``, or a ``DeviceForecastingDataset`` (``origins`` then defaults to
    its index).  Every chunk is one forward in eval mode under ``torch.no_grad()`` followed by one ``EvalMetrics.update`` against channel
    ``target_channel`` of the future window; nothing is read back before the table.  ``scaler``: see ``_scale_shift``.  ``horizons``: the rows
    reported (the reference's ``EVALUATION_HORIZONS``; default all).  Returns an ``EvalResult``, with ``return_predictions=True`` the
    pair ``(EvalResult, normalised predictions [W, H, N] on the device)``.  The ``training`` flag is restored on exit.

    ``per_node=True``: the accumulator is built with the loader's N (``EvalMetrics(nodes=N)``) and the result carries ``per_node``
    [N, len(horizons), 3] and ``per_node_overall`` [N, 3].  ``return_predictions="data"``: the pair's second member holds the
    predictions in the data's units (``pred * std + mean``, bit for bit what torch computes from the normalised ones), stored by the
    per-node launch as it takes the metrics -- no copy and no rescale launch; it implies that launch whatever ``per_node`` is (the
    result's per-node fields are then filled too).  Any other string: ``ValueError``.

    ``process_group`` (a ``torch.distributed`` group every rank of which makes this call with the same arguments): the pass is spread
    over its ranks -- chunk ``c`` is evaluated by rank ``c % world`` (``eval_rank_chunks``) with the composition it has in a
    single-process pass, all ranks draw the graph learner's noise under rank 0's eval seed (one small broadcast), the tables are merged by
    ``EvalMetrics.all_reduce`` and every rank returns the whole pass.  That needs a pass that does not depend on who evaluates what:
    ``model.eval_noise == "window"``; and ``return_predictions=False`` (no rank holds them all).  Either violation raises ``ValueError``
    before any collective.  ``per_node=True`` works: the per-node table is merged in the same collective, every rank returns it whole.  The ranks are taken to hold the same weights AND buffers: data-parallel replicas share their parameters,
    not their BatchNorm running statistics (``step_amd.comm.broadcast_running_statistics`` hands rank 0's to every rank)."""
    from .step_arch.step import DeviceWindowLoader
    if isinstance(return_predictions, str) and return_predictions != "data":
        raise ValueError(f"STEP.evaluate: return_predictions = {return_predictions!r} must be False, True or \"data\"")
    if process_group is not None:
        if getattr(model, "eval_noise", "position") != "window":
            raise ValueError("STEP.evaluate(process_group=...): a pass spread over ranks needs eval_noise = \"window\" (positional noise "
                             "depends on which rank evaluates which batch)")
        if return_predictions:
            raise ValueError("STEP.evaluate(process_group=...): return_predictions is not available for a pass spread over ranks")
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
    in_data_units = return_predictions == "data"
    metrics = EvalMetrics(H, null_val, _scale_shift(scaler), device=dev, nodes=N if per_node or in_data_units else None)
    kept = torch.empty(len(origins), H, N, device=dev) if return_predictions else None
    starts = list(range(0, len(origins), step))
    if process_group is not None:
        import torch.distributed as dist
        seed = [model.eval_seed() if dist.get_rank(process_group) == 0 else None]
        dist.broadcast_object_list(seed, src=dist.get_global_rank(process_group, 0), group=process_group)          # rank 0's eval seed
        starts = [starts[c] for c in eval_rank_chunks(len(starts), dist.get_rank(process_group), dist.get_world_size(process_group))]
        seed_before, model._eval_seed_override = model._eval_seed_override, int(seed[0])
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for at in starts:
                hist, ref, fut = loader.batch(origins[at:at + step])
                pred = model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=None, epoch=None)[0]
                if in_data_units:
                    metrics.update(pred, fut[..., int(target_channel)], out=kept[at:at + pred.shape[0]])
                    continue
                metrics.update(pred, fut[..., int(target_channel)])
                if kept is not None:
                    kept[at:at + pred.shape[0]].copy_(pred[..., 0])
    finally:
        model.train(was_training)
        if process_group is not None:
            model._eval_seed_override = seed_before
    if process_group is not None:
        metrics.all_reduce(process_group)
    res = metrics.result(horizons)
    return (res, kept) if return_predictions else res
