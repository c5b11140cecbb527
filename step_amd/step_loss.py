"""Loss hook with the reference's signature (``step/step_loss/step_loss.py:5-16`` +
``basicts/metrics/mae.py:5-28``): ``step_loss(prediction, real_value, theta, priori_adj,
gsl_coefficient, null_val)``.  The reference runner calls it on RESCALED predictions
(``base_tsf_runner.py:240-250``); it is caller-side code, a handful of element-wise torch ops on
``[B,12,N,1]`` / ``[B,N,N]`` tensors whose autograd feeds ``dpred`` / ``dtheta`` into the native backward.
"""
import ctypes
import hashlib
import numbers

import numpy as np
import torch


def masked_mae(preds, labels, null_val=np.nan):
    if np.isnan(null_val):
        mask = ~torch.isnan(labels)
    else:
        mask = ~((labels - null_val).abs() <= 5e-5)          # ~isclose(labels, null_val, atol=5e-5, rtol=0): a NaN label counts
    mask = mask.float()
    mask = mask / torch.mean(mask)
    mask = torch.nan_to_num(mask, nan=0.0)
    loss = torch.abs(preds - labels) * mask
    return torch.mean(torch.nan_to_num(loss, nan=0.0))


def _flat_stride(x):
    """element stride s such that the logical elements of x, in C order, sit at x.data_ptr() + 4 * s * i (x contiguous: 1; one
    feature of a contiguous [..., C] tensor, ``y[..., :1]``: C); None when x has no such stride."""
    if x.is_contiguous():
        return 1
    if x.dim() < 2 or x.shape[-1] != 1:
        return None
    s = x.stride(-2)
    exp = s
    for d in range(x.dim() - 2, -1, -1):
        if x.shape[d] != 1 and x.stride(d) != exp:
            return None
        exp *= x.shape[d]
    return s


class _NativeStepLoss(torch.autograd.Function):
    """Loss value + both gradients from two HIP launches (libstep_hip step_loss_scaled_fwd_bwd); the backward multiplies both by the
    incoming gradient in one more."""

    @staticmethod
    def forward(ctx, prediction, real_value, theta, priori_adj, coef, null_val, scale, shift):
        from . import _lib
        p = prediction.contiguous().float()
        r = real_value.float()
        rs = _flat_stride(r)
        if rs is None:
            r, rs = r.contiguous(), 1
        t = theta.contiguous().float()
        a = priori_adj.contiguous().float()
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        dp, dt = torch.empty_like(p), torch.empty_like(t)
        work = torch.empty(3, device=p.device, dtype=torch.float64)
        assert r.is_cuda and r.dtype == torch.float32
        if torch.is_tensor(coef):
            # replayed (graph-captured) step: `coef` is the device StepDynState whose gsl_coef field the kernel reads (step_amd/graphed.py)
            _lib.call("step_loss_scaled_fwd_bwd_dyn", _lib.ptr(p), ctypes.c_void_p(r.data_ptr()), p.numel(), rs, float(scale), float(shift), _lib.ptr(t),
                      _lib.ptr(a), t.numel(), float(null_val), _lib.ptr(work), _lib.ptr(loss), _lib.ptr(dp), _lib.ptr(dt), _lib.ptr(coef), _lib.stream())
        else:
            _lib.call("step_loss_scaled_fwd_bwd", _lib.ptr(p), ctypes.c_void_p(r.data_ptr()), p.numel(), rs, float(scale), float(shift), _lib.ptr(t),
                      _lib.ptr(a), t.numel(), float(null_val), float(coef), _lib.ptr(work), _lib.ptr(loss), _lib.ptr(dp), _lib.ptr(dt), _lib.stream())
        ctx.save_for_backward(dp, dt)
        ctx.shapes = (prediction.shape, theta.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        dp, dt = ctx.saved_tensors
        if g.is_cuda and g.dtype == torch.float32 and g.numel() == 1:
            op, ot = torch.empty_like(dp), torch.empty_like(dt)
            _lib.call("step_scale2", _lib.ptr(dp), dp.numel(), _lib.ptr(dt), dt.numel(), _lib.ptr(g.contiguous()), _lib.ptr(op), _lib.ptr(ot),
                      _lib.stream())
        else:
            op, ot = dp * g, dt * g
        return op.view(ctx.shapes[0]), None, ot.view(ctx.shapes[1]), None, None, None, None, None


def _is_nan(x):
    return isinstance(x, numbers.Real) and x != x


def _is_scalar(x):
    """a scaler argument that is one number (a Python / numpy scalar, or a 0-dim array or tensor) rather than N values"""
    return not ((torch.is_tensor(x) or isinstance(x, np.ndarray)) and x.ndim >= 1)


_NODE_SCALERS = {}


def node_scaler(mean, std, N, device, what):
    """``(mean, std)`` of a ``re_standard_transform`` scaler -> None when both are scalars, else ``(scale, shift)``: f32 ``[N]`` device
    tensors of std and mean for ``step_train_tail_nodes`` / ``step_eval_metrics_accumulate_nodes``.  N values may be a numpy array or a
    torch tensor (on any device) whose non-unit dimensions are exactly ``(N,)`` -- ``[1, N, 1]`` as ``standard_transform`` pickles them
    under ``--norm_each_channel``, ``[N]``, ``[N, 1]``; a scalar next to an array is broadcast on the host.  The conversion to f32 and the
    upload happen once per content: the device copies are cached under (device, current stream, digest of the arguments' bytes), keyed
    as the work buffers are."""
    if _is_scalar(mean) and _is_scalar(std):
        return None
    host = []
    for name, x in (("std", std), ("mean", mean)):
        if _is_scalar(x):
            x = np.full(N, float(x), dtype=np.float64)
        else:
            x = x.detach().cpu().numpy() if torch.is_tensor(x) else x
            if tuple(d for d in x.shape if d != 1) not in ((N,), ()) or (x.size == 1 and N != 1):
                raise ValueError(f"{what}: the scaler's {name} has shape {tuple(x.shape)}; N values need non-unit dimensions ({N},)")
            x = np.ascontiguousarray(x).reshape(N)
        host.append(x)
    key = (device.index, torch.cuda.current_stream().cuda_stream, N,
           hashlib.blake2b(b"".join(str(x.dtype).encode() + x.tobytes() for x in host), digest_size=16).digest())
    pair = _NODE_SCALERS.get(key)
    if pair is None:
        if len(_NODE_SCALERS) >= 64:          # (a run has one scaler; a sweep over many does not grow this without bound)
            _NODE_SCALERS.clear()
        vals = [x.astype(np.float32) for x in host]
        if not all(np.isfinite(v).all() for v in vals):
            raise ValueError(f"{what}: the scaler's mean and std must be finite")
        pair = _NODE_SCALERS[key] = tuple(torch.from_numpy(v).to(device) for v in vals)
    return pair


def _through_train_tail(null_val, rescale):
    """what ``_NativeStepLoss`` (the loss kernels of csrc/optim.hip) does not take: a NaN ``null_val``, a per-node scaler"""
    return _is_nan(null_val) or (rescale is not None and not (_is_scalar(rescale[0]) and _is_scalar(rescale[1])))


def step_loss_native(prediction, real_value, theta, priori_adj, gsl_coefficient, null_val=0.0, rescale=None, horizons=None):
    """Same signature and value as ``step_loss``, computed by libstep_hip.
    ``rescale=(mean, std)``: ``prediction`` / ``real_value`` are the NORMALISED tensors and the loss is taken on ``x * std + mean`` --
    the runner's inverse scaling (base_tsf_runner.py:240-250, step_runner.py:86-92) done inside the loss kernels instead of four
    element-wise launches before them and their autograd nodes after; ``real_value`` may be one feature of the batch tensor
    (``future[..., :1]``), it is read in place.
    NaNs follow the reference: a NaN label is not close to ``null_val``, so it counts in the denominator; a NaN ``|p - y|`` adds 0 and has gradient 0.
    ``horizons=k``: the loss of ``train_tail`` on the first ``k`` horizon steps of the FULL tensors (curriculum learning).
    A NaN ``null_val`` (the reference's default: only NaN labels are masked) and a per-node ``rescale`` (arrays of N values, see
    ``node_scaler``) also go through ``train_tail``, over all horizons, with its conditions on the tensors (``[B, H, N, 1]`` or
    ``[B, H, N]``); everything else takes the loss kernels it always took -- also a device-resident ``gsl_coefficient``
    (``GraphedTrainStep``), whose contract stays a finite ``null_val`` and a scalar scaler."""
    if horizons is not None or (_through_train_tail(null_val, rescale) and not torch.is_tensor(gsl_coefficient)):
        return train_tail(prediction, real_value, theta, priori_adj, gsl_coefficient, null_val=null_val, rescale=rescale, horizons=horizons)[0]
    mean, std = (0.0, 1.0) if rescale is None else rescale
    return _NativeStepLoss.apply(prediction, real_value, theta, priori_adj, gsl_coefficient, null_val, std, mean)


def _bhn_strides(x):
    """element strides (b, h, n) of a [B, H, N] / [B, H, N, 1] tensor as libstep_hip takes them (all positive), or None"""
    st = x.stride()[:3]
    return tuple(int(v) for v in st) if all(v >= 1 for v in st) else None


_TAIL_WORK = {}


def _tail_work(device):
    """the work buffer of ``step_train_tail`` of (device, current stream): allocated zeroed once, kept clean by the kernels; two
    streams never share one"""
    from . import _lib
    key = (device.index, torch.cuda.current_stream().cuda_stream)          # (like every call of this package: the current device's stream)
    w = _TAIL_WORK.get(key)
    if w is None:
        w = _TAIL_WORK[key] = torch.zeros(_lib.lib().step_train_tail_work_doubles(), dtype=torch.float64, device=device)
    return w


class _TrainTail(torch.autograd.Function):
    """loss, both gradients and the three meters on the first k horizons from the two launches of libstep_hip step_train_tail; the
    backward multiplies the gradients by the incoming one in one more (step_scale2)"""

    @staticmethod
    def forward(ctx, prediction, real_value, theta, priori_adj, coef, null_val, scale, shift, k):
        from . import _lib
        B, H, N = prediction.shape[:3]
        p, r = prediction.detach(), real_value.detach()
        ps, rs = _bhn_strides(p), _bhn_strides(r)
        if ps is None:
            p = p.contiguous()
            ps = _bhn_strides(p)
        if rs is None:
            r = r.contiguous()
            rs = _bhn_strides(r)
        t = theta.detach().contiguous()
        a = priori_adj.detach().contiguous().float()
        dev = p.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        metrics = torch.empty(3, device=dev, dtype=torch.float32)
        dp = torch.empty((B, H, N), device=dev, dtype=torch.float32)
        dt = torch.empty_like(t)
        if torch.is_tensor(scale):          # a per-node scaler: f32 [N] device tensors of node_scaler
            entry, scaler = "step_train_tail_nodes", (_lib.ptr(scale), _lib.ptr(shift))
        else:
            entry, scaler = "step_train_tail", (float(scale), float(shift))
        _lib.call(entry, ctypes.c_void_p(p.data_ptr()), *ps, ctypes.c_void_p(r.data_ptr()), *rs, B, H, N, int(k), *scaler,
                  float(null_val), _lib.ptr(t), _lib.ptr(a), t.numel(), float(coef), _lib.ptr(_tail_work(dev)), _lib.ptr(loss),
                  _lib.ptr(metrics), _lib.ptr(dp), _lib.ptr(dt), _lib.stream())
        ctx.save_for_backward(dp, dt)
        ctx.shapes = (prediction.shape, theta.shape)
        ctx.mark_non_differentiable(metrics)
        ctx.set_materialize_grads(False)          # (no zeros launch for the metrics' absent gradient)
        return loss, metrics

    @staticmethod
    def backward(ctx, g, _g_metrics):
        from . import _lib
        if g is None:
            return (None,) * 9
        dp, dt = ctx.saved_tensors
        if g.is_cuda and g.dtype == torch.float32 and g.numel() == 1:
            op, ot = torch.empty_like(dp), torch.empty_like(dt)
            _lib.call("step_scale2", _lib.ptr(dp), dp.numel(), _lib.ptr(dt), dt.numel(), _lib.ptr(g.contiguous()), _lib.ptr(op), _lib.ptr(ot),
                      _lib.stream())
        else:
            op, ot = dp * g, dt * g
        return op.view(ctx.shapes[0]), None, ot.view(ctx.shapes[1]), None, None, None, None, None, None


def train_tail(prediction, real_value, theta, priori_adj, gsl_coefficient, null_val=0.0, rescale=None, horizons=None):
    """-> ``(loss, metrics)``: the tail of one training iteration of the reference's runner under curriculum learning
    (base_tsf_runner.py:237-254 with :170-190) from two launches of libstep_hip.  ``loss`` is ``step_loss`` on the first ``horizons``
    horizon steps of ``prediction * std + mean`` / ``real_value * std + mean`` (``rescale=(mean, std)``; None: as they are),
    differentiable w.r.t. ``prediction`` (the gradient has the prediction's FULL shape, exact zeros on the excluded horizons) and
    ``theta``; ``metrics`` is an f32 ``[3]`` tensor (masked MAE, RMSE, MAPE of basicts/metrics on the same slice), no gradient.
    ``prediction`` / ``real_value``: f32 device tensors of one shape ``[B, H, N, 1]`` (or ``[B, H, N]``), NOT sliced; ``real_value`` may
    be one feature of the batch tensor (``future[..., :1]``): it is read in place, nothing is rescaled, sliced or copied.
    ``horizons=None``: all of them.  ``null_val`` may be NaN (the reference's default: the mask is ``~isnan(label)``); an infinite
    one raises ``ValueError``.  ``mean`` and ``std`` may each be a scalar or N values (the per-node scaler of ``--norm_each_channel``,
    see ``node_scaler``): element ``(b, h, n)`` is then taken on ``x * std[n] + mean[n]``; a wrong length raises ``ValueError``.  A tensor
    ``gsl_coefficient`` (the graph-captured step) is not supported here."""
    if torch.is_tensor(gsl_coefficient):
        raise ValueError("train_tail: a device-resident gsl_coefficient (GraphedTrainStep) is not supported")
    if not (torch.is_tensor(prediction) and torch.is_tensor(real_value) and prediction.is_cuda and real_value.is_cuda
            and prediction.dtype == torch.float32 and real_value.dtype == torch.float32 and prediction.shape == real_value.shape
            and (prediction.dim() == 3 or (prediction.dim() == 4 and prediction.shape[3] == 1)) and prediction.numel() > 0):
        raise ValueError("train_tail: prediction and real_value must be f32 device tensors of one shape [B, H, N, 1] or [B, H, N]")
    if not (theta.is_cuda and theta.dtype == torch.float32 and theta.numel() == priori_adj.numel() > 0):
        raise ValueError("train_tail: theta must be an f32 device tensor with as many elements as priori_adj")
    H = prediction.shape[1]
    k = H if horizons is None else int(horizons)
    if not 1 <= k <= H or H > 64:
        raise ValueError(f"train_tail: horizons = {horizons} is not in 1..{H} (at most 64 horizon steps)")
    null_val = float(null_val)
    if null_val in (float("inf"), float("-inf")):
        raise ValueError("train_tail: null_val must be finite or NaN")
    mean, std = (0.0, 1.0) if rescale is None else rescale
    nodes = node_scaler(mean, std, prediction.shape[2], prediction.device, "train_tail")
    scale, shift = (float(std), float(mean)) if nodes is None else nodes
    return _TrainTail.apply(prediction, real_value, theta, priori_adj, float(gsl_coefficient), null_val, scale, shift, k)


def step_loss(prediction, real_value, theta, priori_adj, gsl_coefficient, null_val=np.nan):
    B, N, _ = theta.shape
    t = theta.reshape(B, N * N)
    y = priori_adj.reshape(B, N * N)
    loss_graph = torch.nn.functional.binary_cross_entropy(t, y)
    loss_pred = masked_mae(prediction, real_value, null_val)
    return loss_pred + loss_graph * gsl_coefficient


_DUMMY = {}


def masked_mae_native(preds, labels, null_val=0.0, rescale=None):
    """``masked_mae(preds * std + mean, labels * std + mean, null_val)`` (basicts/metrics/mae.py:5-28 behind the runner's inverse scaling,
    base_tsf_runner.py:240-250) with value and gradient from the two launches of ``step_loss_native`` -- the TSFormer pre-training loss
    (step/TSFormer_*.py: ``CFG.TRAIN.LOSS = masked_mae``).  Element order does not matter to a mean: pass the tensors in whatever
    contiguous layout they have (the pre-training module's outputs are transposed views of contiguous tensors: ``recon.transpose(1, 2)``).
    A NaN ``null_val`` goes through ``train_tail`` (the tensors of any shape, read as one row); a per-node ``rescale`` too, and then
    ``preds`` / ``labels`` must be ``[B, H, N, 1]`` or ``[B, H, N]``: the node is the third dimension."""
    dev = preds.device
    d = _DUMMY.get(dev)
    if d is None:      # the graph term of step_loss with coefficient 0: one edge with theta = prior = 1/2
        d = _DUMMY[dev] = (torch.full((1, 1, 1), 0.5, device=dev), torch.full((1, 1, 1), 0.5, device=dev))
    if _is_nan(null_val) and (rescale is None or (_is_scalar(rescale[0]) and _is_scalar(rescale[1]))):
        preds, labels = preds.reshape(1, 1, -1), labels.reshape(1, 1, -1)
    return step_loss_native(preds, labels, d[0], d[1], 0.0, null_val=null_val, rescale=rescale)


_METRIC_WORK = {}


def masked_metrics_native(preds, labels, null_val=0.0):
    """-> f32 cuda tensor [3] = (masked_mae, masked_rmse, masked_mape) of ``basicts/metrics/{mae,rmse,mape}.py`` for a finite ``null_val``
    (MAPE's own null value is 0, mape.py:21), from ONE launch of libstep_hip instead of ~30 element-wise ones -- the three numbers the
    reference's runner evaluates every training iteration (base_tsf_runner.py:252-254).  No gradient (they feed the epoch meters).
    Its contract stays finite and unscaled: the tensors are the RESCALED ones, and a NaN ``null_val`` does NOT get the reference's
    ``~isnan(labels)`` mask here (``train_tail`` and ``EvalMetrics`` implement it; ``native_runner`` never passes a NaN on)."""
    from . import _lib
    p, r = preds.detach(), labels.detach()
    if p.dtype != torch.float32 or r.dtype != torch.float32 or not p.is_cuda or p.numel() != r.numel():
        raise ValueError("masked_metrics_native: f32 cuda tensors of one size")
    ps, rs = _flat_stride(p), _flat_stride(r)
    if ps is None:
        p, ps = p.contiguous(), 1
    if rs is None:
        r, rs = r.contiguous(), 1
    work = _METRIC_WORK.get(p.device)
    if work is None:
        work = _METRIC_WORK[p.device] = torch.zeros(6, dtype=torch.float64, device=p.device)
    out = torch.empty(3, dtype=torch.float32, device=p.device)
    _lib.call("step_masked_metrics", ctypes.c_void_p(p.data_ptr()), ps, ctypes.c_void_p(r.data_ptr()), rs, p.numel(), float(null_val),
              _lib.ptr(work), _lib.ptr(out), _lib.stream())
    return out
