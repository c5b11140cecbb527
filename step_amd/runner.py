"""BasicTS runner hooks for the native STEP module: the pieces that make the schedule ``bench.py`` times reachable from the
reference's OWN training loop by config lines only ("missing" 3).

The reference's loop (easytorch ``Runner.train`` -> ``BaseTimeSeriesForecastingRunner.train_iters`` -> ``STEPRunner.forward``,
``basicts/runners/base_tsf_runner.py:225-255``, ``step/step_runner/step_runner.py:43-78``) never calls ``STEP.prefetch``, moves
14.9 MB of long history per window across PCIe (``step/step_data/forecasting_dataset.py:52-71``) and reads three metrics back to the
host every iteration (``metric_item.item()``, ``base_tsf_runner.py:253-254``: three device synchronisations per step).  The config
already has the slots to change all of that without touching the loop -- ``CFG.RUNNER`` and ``CFG.DATASET_CLS``
(``step/STEP_PEMS04.py:21-22``):

    from step_amd import STEP
    from step_amd.runner import native_runner, DeviceForecastingDataset
    CFG.RUNNER = native_runner(STEPRunner)            # look-ahead loader + STEP.prefetch, deferred meters, fused clip + Adam
    CFG.DATASET_CLS = DeviceForecastingDataset        # optional: index-only windows over a device-resident series (no PCIe)
    CFG.MODEL.ARCH = STEP

``native_runner(base)`` returns a subclass of the reference's runner class; every hook it overrides calls the reference's own
implementation and only changes WHERE the data lives and WHEN the host reads numbers back:

* ``build_train_data_loader`` / ``build_val_data_loader`` / ``build_test_data_loader`` wrap the loader the reference builds in a
  ``LookaheadLoader``: it holds one batch ahead, puts that batch on the device (pinned memory + an asynchronous copy on its own stream
  for host batches; one gather launch for index batches) and calls ``model.prefetch(next long history)`` BEFORE it hands out the
  current batch -- the frozen TSFormer + kNN prior of batch i + 1 then run next to the whole of step i ("Step schedule").
* the epoch meters are fed once per epoch (when ``print_epoch_meters`` needs them) from values that stayed on the device instead of
  ``.item()`` per iteration, and the three metrics of ``basicts/metrics`` come from one launch (``step_masked_metrics``) instead of
  ~30 element-wise ones; the printed averages are the same numbers.  The feature selections of ``step_runner.py:25-26,39-40`` become
  slices where the feature list is a contiguous range (advanced indexing copies an index tensor to the device: a blocking copy).
* ``init_training`` swaps the ``torch.optim.Adam`` + ``clip_grad_norm_`` pair the config asks for (``STEP_PEMS04.py:89-106``) for
  ``step_amd.optim.FusedAdamClip`` with the same hyper-parameters (one pass over the flat buffers); any other optimizer is left alone.
  What easytorch's ``load_model_resume()`` restored on the replaced pair moves over (``hand_over_training_state``), and the fused
  optimizer's ``state_dict()`` is in torch's Adam format, so checkpoints resume under either runner.

The pre-training stage (``step/TSFormer_*.py``) has the same slots: ``native_runner(TSFormerRunner, native_pretrain=True)`` and
``CFG.DATASET_CLS = DevicePretrainingDataset`` (index-only ``(future_data, LongHistoryRef)`` batches, fused clip + Adam, loss + gradient +
meters of an iteration from one ``TSFormer.pretrain_tail`` call).

The validation pass of the forecasting stage (``base_tsf_runner.py:257-273``: three metric functions and three ``.item()`` per batch of 8
windows) has two switches of its own, both off by default: ``native_eval=True`` takes the ``val_`` meters from one
``step_amd.EvalMetrics`` per pass (one launch per batch, one read-back per pass), ``eval_batch_size=E`` lets the look-ahead loader
concatenate batches of origins so that a validation / test forward carries ``E`` windows.

A launch on several GPUs (``CFG.GPU_NUM = 2``, the reference's default) hands the runner a ``DistributedDataParallel`` wrap, under which
the reducer owns the gradients and all of the above but the loaders is off.  ``native_runner(..., native_data_parallel=True)`` takes the
module out of the wrap in ``init_training`` and calls its ``enable_native_data_parallel()`` (the flat gradient buffer averaged inside
backward), and checks once per epoch that the ranks' parameters are still the same bits (``step_amd.comm.replicas_identical``).
``shard_graph_learner=True`` on top of it cuts STEP's graph learner in time slices over the ranks and gathers them at the end of every
epoch, so that rank 0 validates the whole learner and writes one checkpoint in the reference's format.

Nothing here imports the reference or easytorch: the base class is handed in by the config file, which lives in the reference tree.
"""
import math
import numbers
import os
import pickle

import numpy as np
import torch
from torch.utils.data import Dataset

from .step_arch.step import STEP, DeviceWindowLoader, LongHistoryRef
from .step_arch.tsformer import TSFormer


def _unwrap(model):
    return model.module if hasattr(model, "module") and isinstance(getattr(model, "module"), torch.nn.Module) else model


class DeviceForecastingDataset(Dataset):
    """Drop-in for ``step/step_data/forecasting_dataset.py:8-80`` (same constructor arguments, same files, same length) whose samples
    are FORECAST ORIGINS: ``__getitem__`` returns the int64 scalar ``idx[1]`` of the reference's index triple, the DataLoader's default
    collate makes an int64 ``[B]`` tensor of them, and ``LookaheadLoader`` turns that into ``(future_data, history_data,
    LongHistoryRef)`` with one gather launch over the series, which is moved to the device once.  Windows whose long history would
    start before the series does are all-zero, like the reference's (``forecasting_dataset.py:66-67``)."""

    index_only = True

    def __init__(self, data_file_path, index_file_path, mode, seq_len):
        super().__init__()
        assert mode in ["train", "valid", "test"], "error mode"
        for p, what in ((data_file_path, "data"), (index_file_path, "index")):
            if not os.path.isfile(p):
                raise FileNotFoundError("BasicTS can not find {0} file {1}".format(what, p))
        with open(data_file_path, "rb") as f:
            self.data = torch.from_numpy(pickle.load(f)["processed_data"]).float()
        with open(index_file_path, "rb") as f:
            self.index = pickle.load(f)[mode]
        self.seq_len = int(seq_len)
        first = self.index[0]
        self.history_len, self.future_len = int(first[1] - first[0]), int(first[2] - first[1])
        if self.history_len != self.future_len:
            raise ValueError("DeviceForecastingDataset gathers history and future windows of one length (the STEP configs: 12 -> 12)")
        self._loaders = {}

    def __getstate__(self):          # DataLoader workers get the index and the host series, never the device copies
        d = dict(self.__dict__)
        d["_loaders"] = {}
        return d

    def __getitem__(self, index):
        idx = self.index[index]
        if idx[1] - idx[0] != self.history_len or idx[2] - idx[1] != self.future_len:
            raise ValueError(f"index entry {index} = {tuple(idx)} does not have the dataset's window lengths")
        return torch.tensor(int(idx[1]), dtype=torch.int64)

    def __len__(self):
        return len(self.index)

    def windows(self, origins, device, host_origins=None):
        """int64 [B] forecast origins -> (future_data [B,H,N,C], history_data [B,H,N,C], LongHistoryRef [B,L,N,C]) on ``device``.
        ``host_origins``: the same origins where the caller still holds them on the host (the reference then knows its windows
        without reading the device: STEP's evaluation cache keys on them)"""
        hist, long_ref, fut = self.device_loader(device).batch(origins, t0_host=None if host_origins is None else host_origins.tolist())
        return fut, hist, long_ref

    def device_loader(self, device):
        """the dataset's ``DeviceWindowLoader`` on ``device``: the series is moved there once"""
        key = (device.type, device.index)
        if key not in self._loaders:
            self._loaders[key] = DeviceWindowLoader(self.data.to(device), self.seq_len, self.history_len)
        return self._loaders[key]


class DevicePretrainingDataset(Dataset):
    """Drop-in for the reference's ``PretrainingDataset`` (``step/step_data/pretraining_dataset.py``, which is basicts'
    ``TimeSeriesForecastingDataset``: the same three constructor arguments, the same files, the same length) whose samples are FORECAST
    ORIGINS, like ``DeviceForecastingDataset``'s: ``__getitem__`` returns the int64 scalar ``idx[1]``, and ``LookaheadLoader`` turns a
    batch of them into ``(future_data, LongHistoryRef)`` -- the pair ``TSFormerRunner.forward`` unpacks
    (``step/step_runner/tsformer_runner.py:57``) -- over the series, which is moved to the device once.  The long history of a window
    (2016 or 4032 rows of every sensor, 126 MB per batch of 16 at PEMS-BAY) is never built: ``TSFormer`` gathers its input from the
    reference.  The window lengths are the index's own (``CFG.DATASET_INPUT_LEN`` / ``CFG.DATASET_OUTPUT_LEN`` when it was generated)."""

    index_only = True

    def __init__(self, data_file_path, index_file_path, mode):
        super().__init__()
        assert mode in ["train", "valid", "test"], "error mode"
        for p, what in ((data_file_path, "data"), (index_file_path, "index")):
            if not os.path.isfile(p):
                raise FileNotFoundError("BasicTS can not find {0} file {1}".format(what, p))
        with open(data_file_path, "rb") as f:
            self.data = torch.from_numpy(pickle.load(f)["processed_data"]).float()
        with open(index_file_path, "rb") as f:
            self.index = pickle.load(f)[mode]
        try:
            idx = np.asarray(self.index, dtype=np.int64)
        except (ValueError, TypeError):
            idx = None
        if idx is None or idx.ndim != 2 or idx.shape[1] != 3 or idx.shape[0] == 0:
            # (history start, forecast origin, future end): the history ends where the future starts
            raise ValueError("DevicePretrainingDataset needs an index of (start, origin, end) triples of contiguous windows")
        self.history_len, self.future_len = int(idx[0, 1] - idx[0, 0]), int(idx[0, 2] - idx[0, 1])
        bad = np.nonzero((idx[:, 1] - idx[:, 0] != self.history_len) | (idx[:, 2] - idx[:, 1] != self.future_len))[0]
        if self.history_len <= 0 or self.future_len <= 0 or bad.size:
            which = f"entry {int(bad[0])} = {tuple(int(v) for v in idx[bad[0]])}" if bad.size else f"entry 0 = {tuple(int(v) for v in idx[0])}"
            raise ValueError(f"DevicePretrainingDataset: index {which} does not have the window lengths "
                             f"({self.history_len}, {self.future_len}) of the first entry (both positive)")
        self._loaders = {}

    def __getstate__(self):          # DataLoader workers get the index and the host series, never the device copies
        d = dict(self.__dict__)
        d["_loaders"] = {}
        return d

    def __getitem__(self, index):
        return torch.tensor(int(self.index[index][1]), dtype=torch.int64)

    def __len__(self):
        return len(self.index)

    def windows(self, origins, device, host_origins=None):
        """int64 [B] forecast origins -> (future_data [B,H,N,C], LongHistoryRef [B,L,N,C]) on ``device``; ``host_origins`` as in
        ``DeviceForecastingDataset.windows``"""
        _, long_ref, fut = self.device_loader(device).batch(origins, t0_host=None if host_origins is None else host_origins.tolist())
        return fut, long_ref

    def device_loader(self, device):
        """the dataset's ``DeviceWindowLoader`` on ``device``: the series is moved there once"""
        key = (device.type, device.index)
        if key not in self._loaders:
            self._loaders[key] = DeviceWindowLoader(self.data.to(device), self.history_len, self.future_len)
        return self._loaders[key]


def coalesce_origin_batches(iterable, k):
    """Yields the batches of ``iterable`` -- 1-D int64 tensors of forecast origins -- ``k`` at a time, concatenated in order on the
    host; the last yield holds what is left (fewer batches, and the loader's last batch may itself be short).  ``k = 1`` hands every
    batch through as the object it is."""
    k = int(k)
    if k < 1:
        raise ValueError(f"coalesce_origin_batches: k = {k} must be at least 1")
    if k == 1:
        yield from iterable
        return
    held = []
    for batch in iterable:
        held.append(batch)
        if len(held) == k:
            yield torch.cat(held)
            held = []
    if held:
        yield held[0] if len(held) == 1 else torch.cat(held)


def coalesce_factor(eval_batch_size, loader):
    """how many consecutive batches of ``loader`` make one forward of about ``eval_batch_size`` windows: ``max(1, E // batch_size)``
    where the loader's dataset is index-only (its batches are origins, cheap to concatenate before they are staged) and the loader has
    an integer ``batch_size``; 1 (``eval_batch_size`` is ignored) for anything else"""
    if eval_batch_size is None or loader is None or not getattr(getattr(loader, "dataset", None), "index_only", False):
        return 1
    b = getattr(loader, "batch_size", None)
    if isinstance(b, bool) or not isinstance(b, numbers.Integral) or b < 1:
        return 1
    return max(1, int(eval_batch_size) // int(b))


class LookaheadLoader:
    """Iterates ``loader`` one batch ahead of its consumer (see the module docstring).  ``runner`` supplies the device
    (``to_running_device``) and the model; ``prefetch=False`` only stages the batches on the device.  ``coalesce = k > 1``: ``k``
    consecutive batches of origins of an index-only dataset are concatenated on the host and staged as ONE batch (their host origins
    travel with it as before); ``group_size`` is the wrapped loader's own batch size."""

    def __init__(self, loader, runner, prefetch=True, coalesce=1):
        self.loader, self.runner, self.prefetch = loader, runner, prefetch
        self.dataset = getattr(loader, "dataset", None)
        self.coalesce = int(coalesce)
        if self.coalesce < 1:
            raise ValueError(f"LookaheadLoader: coalesce = {coalesce} must be at least 1")
        if self.coalesce > 1 and not getattr(self.dataset, "index_only", False):
            raise ValueError("LookaheadLoader: only batches of origins (an index-only dataset) can be coalesced")
        self._copy_stream = None
        self.staged_batches = 0
        self.prefetched_batches = 0
        # (rank, world) of an evaluation pass spread over ranks (native_runner(spread_eval=True)): only the batches
        # ``eval_rank_chunks`` gives this rank are staged and handed out -- selected BEFORE staging, each with the composition it has
        # in the whole pass (a coalesced batch is one chunk).  None: every batch
        self.share = None

    def total_batches(self):
        """batches of the whole pass, whoever evaluates them"""
        return -(-len(self.loader) // self.coalesce)

    def __len__(self):
        n = self.total_batches()
        if self.share is None:
            return n
        from .evaluate import eval_rank_chunks
        return len(eval_rank_chunks(n, *self.share))

    @property
    def group_size(self):
        return getattr(self.loader, "batch_size", None)

    def __getattr__(self, name):          # batch_size, sampler, ... of the wrapped loader (easytorch reads a few)
        return getattr(self.__dict__["loader"], name)

    def _device(self):
        p = next(_unwrap(self.runner.model).parameters())
        return p.device

    def _stage(self, batch):
        """host batch -> device batch, without making the host wait: (future, history, long history), or whatever tuple an index-only
        dataset's ``windows`` makes of a batch of origins"""
        dev = self._device()
        self.staged_batches += 1
        if torch.is_tensor(batch) and batch.dim() == 1 and getattr(self.dataset, "index_only", False):
            origins = batch if batch.is_pinned() or batch.is_cuda else batch.pin_memory()
            return self.dataset.windows(origins.to(dev, non_blocking=True), dev, host_origins=None if batch.is_cuda else batch)
        if dev.type != "cuda":
            return batch
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream(dev)
        out = []
        with torch.cuda.stream(self._copy_stream):
            for t in batch:
                if torch.is_tensor(t) and not t.is_cuda:
                    # pinned batches (the reference's loader pins: PIN_MEMORY = True, STEP_PEMS04.py:122) are copied asynchronously; a pageable
                    # one goes as it is -- pinning it here would be one more pass over 119 MB of long history on the host
                    d = t.to(dev, non_blocking=t.is_pinned())
                    d.record_stream(main)
                    out.append(d)
                else:
                    out.append(t)
        done = torch.cuda.Event()
        done.record(self._copy_stream)
        main.wait_event(done)          # queued, not waited for on the host: kernels issued after this point see the batch
        return tuple(out) if isinstance(batch, (tuple, list)) else out[0]

    def _announce(self, staged):
        model = _unwrap(self.runner.model)
        if not (self.prefetch and isinstance(model, STEP) and model.prefetch_enabled and isinstance(staged, (tuple, list)) and len(staged) == 3):
            return
        long_hist = staged[2]
        if not (isinstance(long_hist, LongHistoryRef) or (torch.is_tensor(long_hist) and long_hist.is_cuda)):
            return
        ff = getattr(self.runner, "forward_features", None)
        model.prefetch(long_hist, channel=0 if ff is None else int(ff[0]))
        self.prefetched_batches += 1

    def __iter__(self):
        it = iter(self.loader) if self.coalesce == 1 else coalesce_origin_batches(self.loader, self.coalesce)
        if self.share is not None:
            from .evaluate import eval_rank_chunks
            mine = set(eval_rank_chunks(self.total_batches(), *self.share))
            it = (batch for c, batch in enumerate(it) if c in mine)
        try:
            nxt = self._stage(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            try:
                nxt = self._stage(next(it))
            except StopIteration:
                nxt = None
            if nxt is not None:
                self._announce(nxt)          # batch i + 1's frozen branch is queued before batch i is consumed
            yield cur


def hand_over_training_state(old_optim, old_scheduler, new_optim, scheduler_param=None):
    """What easytorch's ``load_model_resume()`` restored on the optimizer and the scheduler it built (moments, step counts, ``lr`` /
    ``initial_lr``, the scheduler's ``last_epoch``) moves to the optimizer that replaces them: ``new_optim`` loads the old one's
    ``state_dict()``, a scheduler of the old one's type is built around it from ``scheduler_param`` (``CFG.TRAIN.LR_SCHEDULER.PARAM``)
    and loads the old scheduler's ``state_dict()``.  The scheduler's constructor takes ``initial_lr`` from the group where it finds one,
    so its base rate is the run's, not the decayed rate of the resumed epoch.  -> the new scheduler (None without an old one).  The
    old optimizer's state is released here: its owner drops the optimizer itself."""
    new_optim.load_state_dict(old_optim.state_dict())
    new = None
    if old_scheduler is not None:
        new = type(old_scheduler)(new_optim, **(scheduler_param or {}))
        new.load_state_dict(old_scheduler.state_dict())
    for old_group, group in zip(old_optim.param_groups, new_optim.param_groups):
        for k in ("lr", "initial_lr"):          # (the scheduler's constructor takes a step of its own)
            if k in old_group:
                group[k] = old_group[k]
    old_optim.state.clear()
    return new


MIN_SLICE_COLUMNS = 128          # the sliced backward's floor (step_dgl_global_backward_shard): conv2-output columns per rank


def shard_decision(matmul_precision, T2, world, optimizer_swappable):
    """One rank's vote on ``shard_graph_learner`` -- the ranks take the MIN of their votes before anyone slices.  True when the graph
    learner's global branch can be cut in time slices here: the bf16 contraction mode (the sliced backward has no f32 form), every
    slice of ``DiscreteGraphLearning.slice_bounds(T2, world)`` at least ``MIN_SLICE_COLUMNS`` wide (``T2 = train_length - 18``
    conv2-output columns), and the fused optimizer about to be swapped in (the slice's gradient lives in the flat buffer only).
    Anything else: data-parallel with the whole learner on every rank."""
    from .step_arch.discrete_graph_learning import DiscreteGraphLearning
    if matmul_precision != "bf16" or not optimizer_swappable or int(world) < 2:
        return False
    bounds = DiscreteGraphLearning.slice_bounds(int(T2), int(world))
    return min(bounds[r + 1] - bounds[r] for r in range(int(world))) >= MIN_SLICE_COLUMNS


class _Deferred:
    """what a metric returns while the meters are deferred: ``.item()`` hands back the device value instead of waiting for it"""

    def __init__(self, value):
        self.value = value

    def item(self):
        return self


def native_runner(base, prefetch=True, defer_meters=True, fused_optimizer=True, encoder_workgroups=None, native_metrics=True,
                  eval_cache_bytes=0, native_tail=False, native_pretrain=False, native_data_parallel=False, replica_check=True,
                  native_eval=False, eval_batch_size=None, accumulate=1, shard_graph_learner=False, eval_noise="position",
                  native_test=False, spread_eval=False, test_per_node=False):
    """-> subclass of ``base`` (the reference's ``STEPRunner``, or any ``BaseTimeSeriesForecastingRunner``) for ``CFG.RUNNER``.
    ``encoder_workgroups``: compute units of the persistent encoder launch next to the step (None: 160 at 307 nodes / 336 tokens, the
    measured optimum of config C2; 0: one workgroup per sequence) -- only used while batches are prefetched.
    ``eval_cache_bytes``: HBM budget of ``STEP.eval_cache_bytes`` for the validation and test passes (0, the default: off).  With
    ``DeviceForecastingDataset`` the batches carry their origins on the host, and the second and every later ``validate()`` /
    ``test()`` pass over the same windows loads the frozen TSFormer branch instead of computing it (about 130 KB per window at
    PEMS04).
    ``native_tail``: take the loss, its gradients and the three training meters of an iteration from ONE ``step_loss.train_tail`` call
    on the model's normalised prediction and the batch's target view -- no rescale, no ``[:, :cl_length]`` slice, no copy -- also under
    curriculum learning (``CFG.TRAIN.CL``).  Needs a ``STEP`` module on a GPU, the ``re_standard_transform`` scaler with scalar
    mean / std or with the per-node arrays of ``--norm_each_channel`` (``np.ndarray`` of shape ``(1, N, 1)`` or ``(N, 1)``, N the
    prediction's), ``step_loss`` / ``step_loss_native`` as the loss, only the three basicts metrics and a real ``null_val`` that is not
    infinite (NaN, the reference's default, masks nothing but missing labels); anything else takes the base class's path as with
    ``native_tail=False`` (the default).
    ``native_pretrain``: for ``TSFormerRunner`` (``step/TSFormer_*.py``) around a ``TSFormer`` in pre-train mode on a GPU, not wrapped:
    ``init_training`` flattens the module's parameters and swaps ``torch.optim.Adam`` + ``clip_grad_norm_`` for ``FusedAdamClip`` (under
    the conditions of the STEP branch), and ``train_iters`` / ``val_iters`` take the loss, its gradient and the three meters from ONE
    ``TSFormer.pretrain_tail`` call (validation under ``no_grad``, nothing read back).  That needs the ``re_standard_transform`` scaler
    with scalar mean / std (a per-node scaler stays on the base path here), ``masked_mae`` (basicts' or this package's) as the loss,
    only the three basicts metrics, a real ``null_val`` that is not infinite (NaN included) and no ``CFG.TRAIN.CL``; anything else takes the base class's path as with ``native_pretrain=False`` (the default).
    ``native_data_parallel``: for a launch on several GPUs (``CFG.GPU_NUM = 2`` in fifteen of the reference's sixteen ``step/*.py``
    configs), where easytorch wraps the model in ``DistributedDataParallel``.  ``init_training`` -- after easytorch has built Adam and
    the scheduler and resumed a checkpoint -- takes the module out of the wrap and calls its ``enable_native_data_parallel()`` (rank 0's
    resumed state is broadcast, the flat gradient buffer is averaged inside backward over RCCL's C API or ``torch.distributed``), so
    that everything above acts as for one process: the fused optimizer, the native tail, ``native_pretrain``.  It acts only when
    ``torch.distributed`` is initialised with more than one rank and EVERY rank holds a ``STEP``, or a ``TSFormer`` in pre-train mode,
    on a GPU (one MIN all-reduce; otherwise nothing is unwrapped anywhere and rank 0 warns).  Checkpoints keep the reference's keys
    either way.
    ``shard_graph_learner``: where ``native_data_parallel`` acts on a ``STEP`` (a pre-training ``TSFormer`` has no graph learner:
    nothing changes there), every rank keeps one time slice of the graph learner's global branch and the matching columns of
    ``fc.weight`` (``STEP.enable_native_data_parallel(shard_graph_learner=True)``): the 87 MB ``fc.weight`` gradient of STEP_PEMS04
    never enters a collective.  The ranks vote in the same MIN all-reduce (``shard_decision``: bf16 mode, slices of at least 128
    columns, the fused optimizer swappable); if any rank cannot, rank 0 warns and every rank trains with the whole learner.  The
    fused optimizer is built with ``gathered_state=True``, so resumed torch-format moments are cut to the rank's columns.  At the
    end of every epoch ALL ranks gather -- ``fc.weight``, then its two moments onto rank 0 -- before the base class's
    ``on_epoch_end`` (or, for a base without one, before ``save_model``): rank 0's validation and test run the whole learner
    without a collective, and its checkpoint has the reference's keys and torch Adam's format, so it resumes sliced, unsliced, in
    one process or under the reference's runner.  Not together with ``accumulate > 1`` (``init_training`` raises ``ValueError``).
    ``replica_check``: with ``native_data_parallel`` acting, the first iteration of every epoch starts by comparing a 128-bit digest of
    the ranks' flat parameter buffers (``step_amd.comm.replicas_identical``: one kernel, one 32-byte collective, one read-back; with
    ``shard_graph_learner`` acting, of the replicated part in front of the ``fc.weight`` slice, which has no replica); every
    rank raises ``RuntimeError`` when they differ -- only rank 0 writes the checkpoint, and no wrapper guarantees identical replicas.
    The buffer is the one the fused optimizer updates: where ``init_training`` keeps torch's optimizer there is none and nothing is
    checked.
    ``native_eval``: the validation meters of the forecasting stage come from one ``step_amd.EvalMetrics`` per pass -- ``val_iters``
    queues ONE accumulate launch on the model's normalised prediction and the batch's target view (no rescale, no metric functions, no
    ``.item()``), and ``flush_meters`` reads the mean of the per-batch values back once per pass, before ``save_best_model`` looks at
    ``val_MAE``.  Needs a ``STEP`` module on a GPU, the ``re_standard_transform`` scaler with scalar mean / std or per-node arrays (as for
    ``native_tail``), only the three basicts metrics and a real ``null_val`` (NaN included); anything else takes the base class's ``val_iters`` as with ``native_eval=False``
    (the default).  Under ``native_pretrain`` the runner's ``test()`` (``TSFormerRunner.test``) likewise takes the three ``test_``
    meters of a batch from one ``pretrain_tail`` call and reads nothing back before the meters are printed.
    ``eval_batch_size``: ``E`` windows per validation / test forward instead of the config's ``VAL/TEST.DATA.BATCH_SIZE``: the look-ahead
    loader concatenates ``max(1, E // batch_size)`` consecutive batches of origins before it stages them, ``native_eval`` still
    accumulates per loader batch (the ``val_`` meters stay the mean over the config's batches, ``n`` their count), and the reference's
    ``test()`` evaluates the concatenation of whatever arrives.  Only for index-only datasets (``DeviceForecastingDataset``) behind a
    loader with an integer ``batch_size`` -- ignored otherwise, and never applied to a ``TSFormer``'s loaders (a pre-training forward
    draws one mask).  Off by default (None) because it is not the same pass: the graph learner samples in eval mode too, its Gumbel
    noise is a function of the forward count and the position in the batch, so a coalesced pass draws other noise than the uncoalesced
    one -- as another seed would.
    ``accumulate``: ``k`` iterations per optimizer step (default 1: easytorch's ``backward`` as it is).  Fifteen of the reference's
    sixteen ``step/*.py`` configs set ``CFG.GPU_NUM = 2`` with a per-process batch size: on one card that update is ``accumulate=2``.
    Groups are runs of ``k`` consecutive iterations of an epoch, the last one of an epoch possibly shorter (size ``s``).  At the start
    of a group ``train_iters`` calls ``optim.zero_grad()`` and the module's ``set_grad_accumulation(s)``; ``backward(loss)`` runs
    ``(loss / s).backward()`` and, after the group's last iteration, ``optim.step()`` -- the clip stays inside the fused pass, the
    scheduler and the step count advance per optimizer step, the meters stay per iteration.  It needs the fused optimizer:
    ``init_training`` raises ``RuntimeError`` when ``accumulate > 1`` and ``FusedAdamClip`` was not swapped in (another optimizer, a
    module still wrapped, not a native module on a GPU) rather than train with another effective batch size.  Works with
    ``native_tail``, ``native_pretrain`` and ``native_data_parallel`` (collectives on a group's last backward only).
    ``eval_noise``: ``"window"`` sets ``STEP.eval_noise = "window"`` where the validation / test loaders are built: in eval mode the graph
    learner's Gumbel noise is keyed by (edge, forecast origin of the window, one fixed seed) instead of (edge, position in the batch,
    forward count), so a validation / test pass is a function of the weights and the windows alone -- the same for any
    ``eval_batch_size``, with or without ``eval_cache_bytes``, on any number of ranks, and every epoch's ``val_MAE`` is drawn under the
    same noise.  Needs index-only validation and test datasets (``DeviceForecastingDataset``: the origins are the keys); with anything
    else rank 0 warns and the positional noise stays.  ``"position"`` (default): as the module does by itself.  Anything else:
    ``ValueError``.
    ``native_test``: the forecasting ``test()`` (``base_tsf_runner.py:277-318``: every prediction of the pass kept, concatenated,
    rescaled and sliced per horizon) feeds every batch to one ``step_amd.EvalMetrics`` instead -- one launch per batch, nothing
    concatenated, ONE read-back -- logs the reference's line for each of ``self.evaluation_horizons`` and sets ``test_MAE`` /
    ``test_RMSE`` / ``test_MAPE`` from the table's overall row.  Under the conditions of ``native_eval`` (a ``STEP`` on a GPU, the
    ``re_standard_transform`` scaler with scalar mean / std or per-node arrays, only the three basicts metrics, a real ``null_val``); anything else takes
    the base class's ``test()``.  The pre-training branch of ``test()`` is not affected.
    ``spread_eval``: where ``native_data_parallel`` acts on a ``STEP``, the validation and the test pass of an epoch's end are spread
    over the ranks instead of running on rank 0 while the others wait: batch ``c`` of a pass is evaluated by rank ``c % world``
    (``step_amd.evaluate.eval_rank_chunks``), with the composition it has in the whole pass.  Rank 0 stays the master and runs the
    reference's flow untouched (``validate``, ``test_process``, the meters, ``save_best_model``, ``save_model``) over its share; the
    other ranks build their own validation / test loaders in ``init_training`` and run their share inside ``on_epoch_end``, for the
    passes due this epoch (``VAL.INTERVAL`` / ``TEST.INTERVAL``), in eval mode under ``no_grad``.  Each pass has exactly ONE collective
    per rank, ``EvalMetrics.all_reduce``: the meters rank 0 prints and the ``val_MAE`` ``save_best_model`` reads are those of the whole
    pass.  In front of the passes of an epoch's end every rank takes rank 0's BatchNorm running statistics (one small broadcast,
    ``step_amd.comm.broadcast_running_statistics``): the ranks' own drift apart with their batches, and the pass is rank 0's -- as
    under ``DistributedDataParallel``, which hands rank 0's buffers to every rank.  It needs, on EVERY rank (one more word in the MIN all-reduce of ``init_training``; otherwise rank 0 warns and the passes
    stay master-only): ``native_eval`` and ``native_test`` usable, index-only validation and test datasets, and
    ``eval_noise="window"`` in effect -- only then is a pass the same whoever evaluates which batch.  Rank 0's eval seed is broadcast
    once.  With ``shard_graph_learner`` acting the passes run behind the gather of the slices.  A validation forward whose outputs
    do not qualify for ``EvalMetrics`` raises instead of taking the torch path (the other ranks would wait in the collective).
    Without ``native_data_parallel``, or in a single process, the switch does nothing.
    ``test_per_node``: with ``native_test`` acting, the test pass's ``EvalMetrics`` is built with ``nodes=`` the model's node count (on
    every rank of a spread pass, also one without a batch: all ranks reduce the same number of doubles), rank 0 keeps the pass's
    ``EvalResult`` -- ``per_node`` [N, H, 3] and ``per_node_overall`` [N, 3] filled -- as ``self.test_result`` and logs ONE more line
    behind the reference's per-horizon lines: the five sensors with the largest overall MAE and their values.  The lines, the three
    ``test_`` meters and the single read-back of the pass are as without it.  Where ``native_test`` is not in effect the switch does
    nothing and rank 0 warns once.  The validation meters and the pre-training stage have no per-sensor tables.  Off by default."""
    import operator
    if eval_noise not in ("position", "window"):
        raise ValueError(f"native_runner: eval_noise must be \"position\" or \"window\", got {eval_noise!r}")
    if isinstance(accumulate, (bool, float)) or operator.index(accumulate) < 1:
        raise ValueError(f"native_runner: accumulate must be an integer >= 1, got {accumulate!r}")
    accumulate = operator.index(accumulate)

    class NativeRunner(base):
        native_hooks = True

        def __init__(self, cfg):
            super().__init__(cfg)
            self._deferring = False
            self._pending = {}          # meter name -> [(device value, n), ...] since the last flush
            self._metric_cache = None
            self._dp_acting = False          # native_data_parallel took the module out of its DistributedDataParallel wrap
            self._shard_acting = False          # ... and shard_graph_learner cut the graph learner in time slices
            self._val_metrics = None          # native_eval: (what it was built for, the validation pass's EvalMetrics)
            self._eval_index_only = {}          # eval_noise: "val" / "test" -> the loader built here has an index-only dataset
            self._eval_noise_warned = False
            self._spread_acting = False          # spread_eval: the validation / test passes are spread over the ranks
            self._helper_loaders = {}          # ... on a rank other than 0: its own "val" / "test" loaders
            self.eval_readbacks = 0          # device-to-host copies of EvalMetrics tables (one per pass)
            self.test_result = None          # test_per_node: the EvalResult of the last native test pass (rank 0)
            self._per_node_warned = False
            self._group_size, self._group_pos = 1, 0          # accumulate: size of the open group, iterations of it that ran backward

        # ---------------------------------------------------------------- loaders
        def _lookahead(self, loader, on):
            return LookaheadLoader(loader, self, prefetch=on) if loader is not None else None

        def build_train_data_loader(self, cfg):
            loader = self._lookahead(super().build_train_data_loader(cfg), prefetch)
            model = _unwrap(self.model)
            if prefetch and isinstance(model, STEP) and next(model.parameters()).is_cuda:
                n = encoder_workgroups
                if n is None:
                    n = 160 if (model.backend.num_nodes, int(model.tsformer.num_token)) == (307, 336) else 0
                model.tsformer.encoder_workgroups = int(n)
                model.prefetch_knn_stream = int(n) > 0          # (the look-ahead loader announces at the start of the step: bench.py's policy)
            return loader

        def _enable_eval_cache(self):
            model = _unwrap(self.model)
            if eval_cache_bytes > 0 and isinstance(model, STEP):
                model.eval_cache_bytes = int(eval_cache_bytes)

        def _eval_lookahead(self, loader):
            """the validation / test loader: staged, not announced; ``eval_batch_size`` coalesces origin batches -- never a
            pre-training loader's (one forward of a TSFormer in pre-train mode draws ONE mask for all its windows)"""
            if loader is None:
                return None
            k = 1 if isinstance(_unwrap(self.model), TSFormer) else coalesce_factor(eval_batch_size, loader)
            return LookaheadLoader(loader, self, prefetch=False, coalesce=k)

        def _enable_eval_noise(self, which, loader):
            """eval_noise="window": on the module once the loaders built so far all have index-only datasets (their origins are the keys)"""
            model = _unwrap(self.model)
            if eval_noise != "window" or not isinstance(model, STEP):
                return
            self._eval_index_only[which] = bool(getattr(getattr(loader, "dataset", None), "index_only", False))
            ok = all(self._eval_index_only.values())
            if not ok and not self._eval_noise_warned and self._rank_world()[0] == 0:
                import warnings
                self._eval_noise_warned = True
                warnings.warn("step_amd.runner: eval_noise=\"window\" needs index-only validation and test datasets "
                              "(DeviceForecastingDataset); the graph learner's eval noise stays positional")
            model.eval_noise = "window" if ok else "position"

        @staticmethod
        def _rank_world():
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                return dist.get_rank(), dist.get_world_size()
            return 0, 1

        def build_val_data_loader(self, cfg):
            self._enable_eval_cache()
            loader = self._eval_lookahead(super().build_val_data_loader(cfg))
            self._enable_eval_noise("val", loader)
            return loader

        def build_test_data_loader(self, cfg):
            self._enable_eval_cache()
            loader = self._eval_lookahead(super().build_test_data_loader(cfg))
            self._enable_eval_noise("test", loader)
            return loader

        # ---------------------------------------------------------------- feature selection without a host-device synchronisation
        # ``data[:, :, :, [0, 1, 2]]`` (step_runner.py:25-26,39-40) builds an index tensor on the host and copies it to the device: a blocking
        # copy behind everything queued on the stream, twice per iteration.  For the feature lists the STEP configs use -- contiguous
        # ranges -- a slice selects the same values as a VIEW: no index tensor, no copy, and forward() sees the very tensor the loader
        # announced to STEP.prefetch.  Any other list goes through the reference's indexing (and ``alias_batch``).
        @staticmethod
        def _range_of(features):
            if features is None:
                return None
            f = [int(i) for i in features]
            return (f[0], f[0] + len(f)) if f and f == list(range(f[0], f[0] + len(f))) else None

        def select_input_features(self, data):
            ff = getattr(self, "forward_features", None)
            if isinstance(data, LongHistoryRef):
                return data if ff is None else data[:, :, :, list(ff)]
            r = self._range_of(ff)
            if r is not None and torch.is_tensor(data) and data.dim() == 4 and r[1] <= data.shape[3]:
                out = data[:, :, :, r[0]:r[1]]
                if r[0] != 0 and data.is_cuda and isinstance(_unwrap(self.model), STEP):
                    _unwrap(self.model).alias_batch(data, out, channel=r[0])          # (a view that starts at another channel: another address)
                return out
            out = super().select_input_features(data)
            if out is not data and torch.is_tensor(out) and torch.is_tensor(data) and data.is_cuda:
                model = _unwrap(self.model)
                if isinstance(model, STEP):
                    # advanced indexing made a copy: tell the module that it is the batch the loader announced (same values in the
                    # channel the TSFormer reads), so that forward() finds the prefetched branch
                    model.alias_batch(data, out, channel=0 if ff is None else int(ff[0]))
            return out

        def select_target_features(self, data):
            r = self._range_of(getattr(self, "target_features", None))
            if r is not None and torch.is_tensor(data) and data.dim() == 4 and r[1] <= data.shape[3]:
                return data[:, :, :, r[0]:r[1]]
            return super().select_target_features(data)

        # ---------------------------------------------------------------- optimizer
        def _pretrain_module(self):
            """the TSFormer that ``native_pretrain`` acts on, or None"""
            model = self.model
            ok = (native_pretrain and isinstance(model, TSFormer) and model.mode == "pre-train" and next(model.parameters()).is_cuda)
            return model if ok else None

        def _spread_loaders(self, cfg):
            """this rank's validation and test loaders for a spread pass: rank 0's are the runner's own (init_validation / init_test are
            master-only), the other ranks build theirs through the same hooks -> (val, test), None where there is none"""
            if self._rank_world()[0] == 0:
                return getattr(self, "val_data_loader", None), getattr(self, "test_data_loader", None)
            for which, build in (("val", self.build_val_data_loader), ("test", self.build_test_data_loader)):
                if which not in self._helper_loaders:
                    try:
                        self._helper_loaders[which] = build(cfg)
                    except Exception:          # (a config without that pass, a missing file: this rank votes against)
                        self._helper_loaders[which] = None
            return self._helper_loaders.get("val"), self._helper_loaders.get("test")

        def _spread_vote(self, cfg, model):
            """this rank's vote on spread_eval: native_eval and native_test usable, index-only validation and test datasets behind the
            look-ahead loader, eval_noise="window" in effect"""
            if not (native_eval and native_test and eval_noise == "window" and isinstance(model, STEP) and self._eval_scaler() is not None):
                return False
            loaders = self._spread_loaders(cfg)
            if not all(isinstance(ld, LookaheadLoader) and getattr(ld.dataset, "index_only", False) for ld in loaders):
                return False
            return model.eval_noise == "window"

        def _enable_data_parallel(self, cfg=None):
            """native_data_parallel: the same decision on every rank, then unwrap and enable -> True when it acted"""
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
                return False
            model = _unwrap(self.model)
            able = ((isinstance(model, STEP) or (isinstance(model, TSFormer) and model.mode == "pre-train"))
                    and next(model.parameters()).is_cuda)
            # a mixed decision would deadlock the first collective: one MIN all-reduce before anyone acts
            dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
            votes = [1 if able else 0]
            if shard_graph_learner:
                # the same collective carries the vote on the time slices: no rank may reach shard_time_slices alone
                slices = able and isinstance(model, STEP) and shard_decision(
                    model.matmul_precision, model.discrete_graph_learning.train_length - 18, dist.get_world_size(),
                    self._fused_swap_ok(model, getattr(self, "optim", None), False))
                votes.append(1 if slices else 0)
            if spread_eval:
                # ... and the vote on the spread validation / test passes: no rank may wait in a pass's collective alone
                votes.append(1 if (able and self._spread_vote(cfg, model)) else 0)
            every = torch.tensor(votes, dtype=torch.int32, device=dev)
            dist.all_reduce(every, op=dist.ReduceOp.MIN)
            every = every.tolist()
            spread = bool(spread_eval and every[0] == 1 and every[-1] == 1)
            if spread_eval and not spread:
                self._helper_loaders = {}
                if dist.get_rank() == 0:
                    import warnings
                    warnings.warn("step_amd.runner: spread_eval needs, on every rank, native_data_parallel acting on a STEP, native_eval and "
                                  "native_test usable, index-only validation and test datasets and eval_noise=\"window\"; the validation "
                                  "and test passes stay on rank 0")
            if every[0] == 0:
                if dist.get_rank() == 0:
                    import warnings
                    warnings.warn("step_amd.runner: native_data_parallel needs a STEP, or a TSFormer in pre-train mode, on a GPU on every "
                                  "rank; the model stays in its DistributedDataParallel wrap")
                return False
            if self.model is not model:
                # no reference to the wrapper is kept: its reducer takes its autograd hooks with it.  The optimizer easytorch built holds
                # the same Parameter objects, and save_model / load_model_resume branch on the wrap themselves
                self.model = model
                import gc
                gc.collect()
            if shard_graph_learner and isinstance(model, STEP) and every[1] == 0:
                if dist.get_rank() == 0:
                    import warnings
                    warnings.warn("step_amd.runner: shard_graph_learner needs, on every rank, matmul_precision = 'bf16', time slices of "
                                  f"at least {MIN_SLICE_COLUMNS} columns and the fused optimizer (fused_optimizer=True around a plain "
                                  "torch.optim.Adam with one parameter group and a 2-norm clip); every rank trains data-parallel with "
                                  "the whole graph learner")
            if shard_graph_learner and every[1] == 1:
                # (after the resume: the slice is cut from the resumed, broadcast fc.weight)
                model.enable_native_data_parallel(collectives="auto", sync_module_states=True, shard_graph_learner=True)
                self._shard_acting = True
            else:
                model.enable_native_data_parallel(collectives="auto", sync_module_states=True)          # (after the resume: resumed weights are broadcast)
            if spread:
                self._enable_spread(cfg, model)
            return True

        def _enable_spread(self, cfg, model):
            """every rank, after the vote: this rank's share on its loaders, rank 0's eval seed everywhere (one broadcast)"""
            import torch.distributed as dist
            rank, world = dist.get_rank(), dist.get_world_size()
            for loader in self._spread_loaders(cfg):
                loader.share = (rank, world)
            seed = [model.eval_seed() if rank == 0 else None]
            dist.broadcast_object_list(seed, src=0)
            model._eval_seed_override = int(seed[0])
            self._spread_acting = True

        def init_training(self, cfg):
            if native_data_parallel and shard_graph_learner and accumulate > 1:
                # the module refuses a group of backwards over time slices; said here, by the options' names, on every rank alike
                raise ValueError(f"step_amd.runner: shard_graph_learner=True cannot be combined with accumulate={accumulate}: a time-sliced "
                                 "graph learner takes one backward per optimizer step (set accumulate=1, or shard_graph_learner=False)")
            super().init_training(cfg)
            self._dp_acting = self._enable_data_parallel(cfg) if native_data_parallel else False
            model = _unwrap(self.model)
            opt = getattr(self, "optim", None)
            pretrain = self._pretrain_module() is not None
            self._swap_optimizer(cfg, model, opt, pretrain)
            from .optim import FusedAdamClip
            if accumulate > 1 and not isinstance(self.optim, FusedAdamClip):
                raise RuntimeError(f"step_amd.runner: accumulate={accumulate} needs the fused optimizer, which was not swapped in (it takes "
                                   "fused_optimizer=True, a STEP -- or, with native_pretrain, a pre-training TSFormer -- on a GPU outside "
                                   "any wrapper, and a plain torch.optim.Adam with one parameter group and a 2-norm clip): training on "
                                   "with another effective batch size would be silent")

        def _fused_swap_ok(self, model, opt, pretrain):
            """what ``_swap_optimizer`` asks of the bare module, the optimizer and the clip (the vote on the time slices asks the same
            while the module is still wrapped)"""
            if not (fused_optimizer and (isinstance(model, STEP) or pretrain) and type(opt) is torch.optim.Adam
                    and next(model.parameters()).is_cuda):
                return False
            g = opt.param_groups[0]
            if len(opt.param_groups) != 1 or g.get("amsgrad") or g.get("maximize"):
                return False
            clip = getattr(self, "clip_grad_param", None) or {}
            return not (clip and float(clip.get("norm_type", 2.0)) != 2.0)

        def _swap_optimizer(self, cfg, model, opt, pretrain):
            # (under a DistributedDataParallel wrap the reducer owns the .grad tensors: torch's optimizer stays)
            if not (model is self.model and self._fused_swap_ok(model, opt, pretrain)):
                if self._shard_acting:
                    raise RuntimeError("step_amd.runner: the graph learner is in time slices but the fused optimizer was not swapped in")
                return
            from .optim import FusedAdamClip
            g = opt.param_groups[0]
            clip = getattr(self, "clip_grad_param", None) or {}
            if pretrain:
                model.flatten_parameters()          # (values and state_dict unchanged: every parameter becomes a view into one buffer)
            # positions in the replaced Adam's own list are the indices of the optimizer state on disk, whether easytorch handed it
            # model.parameters() or only the trainable ones
            fused = FusedAdamClip(model, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"],
                                  max_norm=clip.get("max_norm"), param_grads=pretrain, params=g["params"],
                                  gathered_state=self._shard_acting)
            sched = getattr(self, "scheduler", None)
            s = cfg["TRAIN"].get("LR_SCHEDULER") if sched is not None else None
            self.scheduler = hand_over_training_state(opt, sched, fused, s["PARAM"] if s is not None else None)
            self.optim, self.clip_grad_param = fused, None          # the clip is part of the fused pass
            del opt, g, sched          # the last references to the replaced Adam (its moments: two copies of the parameters)

        # ---------------------------------------------------------------- gradient accumulation (accumulate=k)
        def _group_start(self, iter_index):
            """an iteration that opens a group: the group's size, zero_grad(), and the module is told how many backwards follow"""
            if iter_index % accumulate != 0:
                return
            try:
                left = len(self.train_data_loader) - int(iter_index)
            except TypeError:
                left = accumulate          # (a loader without a length: full groups)
            s = max(1, min(accumulate, left))
            self.optim.zero_grad()
            _unwrap(self.model).set_grad_accumulation(s)
            self._group_size, self._group_pos = s, 0

        def backward(self, loss):
            if accumulate == 1:
                return super().backward(loss)
            s = self._group_size
            (loss / s).backward()
            self._group_pos += 1
            if self._group_pos == s:
                self.optim.step()          # (clip_grad_param is None: the clip is part of the fused pass)

        # ---------------------------------------------------------------- meters without a device synchronisation per iteration
        def _check_replicas(self, epoch):
            """every rank runs train_iters (validation and its hooks run on rank 0 only): all ranks see the same answer and raise together.
            Without a flat parameter buffer (the fused optimizer was not swapped in: the same config decision on every rank) there is
            nothing to digest and nothing is checked.  With the graph learner in time slices the buffer ends in this rank's ``fc.weight``
            slice, which differs between the ranks by design and has no replica to be compared against: only the replicated prefix --
            everything in front of the layout's ``norm_slot``, the same length on every rank -- is digested"""
            import torch.distributed as dist
            from .comm import replicas_identical
            model = _unwrap(self.model)
            flat = model._flat_param
            if flat is not None and self._shard_acting:
                flat = flat[:model._grad_layout()["norm_slot"]]
            if flat is not None and not replicas_identical(flat):
                raise RuntimeError(f"step_amd.runner: the data-parallel replicas differ at the start of epoch {epoch} (rank "
                                   f"{dist.get_rank()} of {dist.get_world_size()}): the ranks' flat parameter buffers do not hold the same "
                                   "bits, so the checkpoint rank 0 writes is not what the other ranks trained")

        def train_iters(self, epoch, iter_index, data):
            if self._dp_acting and replica_check and iter_index == 0:
                self._check_replicas(epoch)
            if accumulate > 1:
                self._group_start(iter_index)
            self._deferring, self._metric_cache = defer_meters, None
            try:
                scaler = self._tail_scaler() if native_tail else None
                if scaler is not None:
                    return self._native_tail_iters(epoch, iter_index, data, scaler)
                scaler = self._pretrain_scaler(data) if native_pretrain else None
                if scaler is not None:
                    loss, three = self._pretrain_tail(data, scaler)
                    for metric_name, metric_func in self.metrics.items():
                        self.update_epoch_meter("train_" + metric_name, _Deferred(three[self._NATIVE_METRICS[metric_func.__name__]]))
                    return loss
                return super().train_iters(epoch, iter_index, data)
            finally:
                self._deferring, self._metric_cache = False, None

        _NATIVE_METRICS = {"masked_mae": 0, "masked_rmse": 1, "masked_mape": 2}

        # ---------------------------------------------------------------- the iteration's tail from one native call (native_tail=True)
        def _is_basicts_metric(self, f):
            return (getattr(f, "__name__", None) in self._NATIVE_METRICS
                    and str(getattr(f, "__module__", "")).startswith("basicts.metrics"))

        def _tail_scaler(self):
            """(mean, std) when everything known BEFORE the forward pass allows the native tail, else None"""
            model = _unwrap(self.model)
            if not (isinstance(model, STEP) and next(model.parameters()).is_cuda):
                return None
            return self._scalar_rescale(("step_loss", "step_loss_native"))

        def _scaler_mean_std(self):
            """(mean, std) of a ``re_standard_transform`` scaler: floats for scalar real arguments; the arrays themselves for two
            ``np.ndarray`` of one shape ``(1, N, 1)`` or ``(N, 1)`` -- what ``standard_transform`` pickles under ``--norm_each_channel``
            and ``re_standard_transform`` (basicts/data/transform.py:59-65) broadcasts per node against ``[B, H, N, 1]``.  Anything else
            is None (the base path): torch tensors, a scalar next to an array (the reference fails on it), and shape ``(N,)``, which the
            reference broadcasts against the LAST dimension"""
            scaler = getattr(self, "scaler", None)
            if not isinstance(scaler, dict):
                return None
            func, args = scaler.get("func"), scaler.get("args") or {}
            if getattr(func, "__name__", func) != "re_standard_transform":
                return None
            mean, std = args.get("mean"), args.get("std")
            if isinstance(mean, np.ndarray) and isinstance(std, np.ndarray):
                per_node = mean.shape == std.shape and (mean.ndim == 2 or (mean.ndim == 3 and mean.shape[0] == 1)) and mean.shape[-1] == 1
                if not (per_node and mean.size > 0 and all(x.dtype.kind == "f" and np.isfinite(x).all() for x in (mean, std))):
                    return None
                return mean, std
            if isinstance(mean, bool) or isinstance(std, bool) or not (isinstance(mean, numbers.Real) and isinstance(std, numbers.Real)):
                return None
            return float(mean), float(std)

        @staticmethod
        def _scaler_fits(scaler, pred):
            """a per-node scaler has as many nodes as the forward's ``[B, H, N, 1]`` prediction (scalars fit anything)"""
            mean = scaler[0]
            return not isinstance(mean, np.ndarray) or (torch.is_tensor(pred) and pred.dim() == 4 and mean.size == pred.shape[2])

        @staticmethod
        def _rescaled(x, mean, std):
            """``re_standard_transform`` on torch ops (basicts/data/transform.py:59-65), for the tails that run after a forward whose
            outputs the native calls cannot take"""
            if isinstance(mean, np.ndarray):
                mean = torch.from_numpy(mean).type_as(x).to(x.device).unsqueeze(0)
                std = torch.from_numpy(std).type_as(x).to(x.device).unsqueeze(0)
            return x * std + mean

        def _only_basicts_metrics(self):
            metrics = getattr(self, "metrics", None)
            return isinstance(metrics, dict) and all(self._is_basicts_metric(f) for f in metrics.values())

        def _scalar_rescale(self, loss_names):
            """(mean, std) of ``_scaler_mean_std`` (scalars, or per-node arrays) when the loss is one of ``loss_names``, the metrics are
            the three of basicts and ``null_val`` is a real number that is not infinite (NaN, the reference's default, is allowed; a
            ``bool`` is not), else None"""
            scaler = self._scaler_mean_std()
            if scaler is None or getattr(self.loss, "__name__", None) not in loss_names or not self._only_basicts_metrics():
                return None
            nv = getattr(self, "null_val", 0.0)
            if isinstance(nv, bool) or not isinstance(nv, numbers.Real) or math.isinf(nv):
                return None
            return scaler

        # ---------------------------------------------------------------- validation meters on the device (native_eval=True)
        def _eval_scaler(self):
            """(mean, std) when everything known BEFORE the forward pass allows the validation meters to come from ``EvalMetrics``,
            else None.  The loss plays no part in a validation pass, and ``null_val`` may be NaN (the reference's default)"""
            return self._eval_conditions() if native_eval else None

        def _eval_conditions(self):
            """what ``native_eval`` and ``native_test`` ask for, apart from their switches -> (mean, std) or None"""
            model = _unwrap(self.model)
            if not (isinstance(model, STEP) and next(model.parameters()).is_cuda):
                return None
            scaler = self._scaler_mean_std()
            nv = getattr(self, "null_val", 0.0)
            if scaler is None or not self._only_basicts_metrics() or isinstance(nv, bool) or not isinstance(nv, numbers.Real):
                return None
            return scaler

        def _val_accumulator(self, horizons, mean, std, device):
            """the pass's ``EvalMetrics``: made on first use, kept over the epochs, made anew when what it was built for changes"""
            # (arrays do not compare as keys do: a per-node scaler is told apart by the arrays' identity and shape -- the runner holds
            # them for its lifetime -- a scalar one by its values)
            ident = tuple((id(x), x.shape) if isinstance(x, np.ndarray) else x for x in (std, mean))
            key = (int(horizons), repr(float(self.null_val)), ident, device)
            if self._val_metrics is None or self._val_metrics[0] != key:
                self._drain_val_metrics()          # (nothing to drain unless the key changed in the middle of a pass)
                from .evaluate import EvalMetrics
                self._val_metrics = (key, EvalMetrics(horizons, float(self.null_val), rescale=(std, mean), device=device))
            return self._val_metrics[1]

        def _drain_val_metrics(self):
            """the pass's single device-to-host copy: the mean of the per-batch values goes to the ``val_`` meters"""
            m = self._val_metrics[1] if self._val_metrics is not None else None
            if m is None or m.batches == 0:
                return
            if self._spread_acting:
                # the pass's one collective (rank 0 owns batch 0: it is here whenever the pass has a batch; the others: _helper_passes)
                m.all_reduce(_unwrap(self.model)._process_group)
            res = m.result()
            self.eval_readbacks += 1
            for metric_name, metric_func in self.metrics.items():
                super().update_epoch_meter("val_" + metric_name, float(res.batch_mean[self._NATIVE_METRICS[metric_func.__name__]]), n=res.batches)
            m.reset()

        @staticmethod
        def _qualifies(pred, real):
            """the forward's outputs are what ``EvalMetrics.update`` takes"""
            from .evaluate import MAX_HORIZONS
            return (torch.is_tensor(pred) and torch.is_tensor(real) and pred.is_cuda and real.is_cuda and pred.device == real.device
                    and pred.dtype == torch.float32 and real.dtype == torch.float32 and pred.dim() == 4 and pred.shape[3] == 1
                    and pred.shape == real.shape and 0 not in pred.shape and pred.shape[1] <= MAX_HORIZONS
                    and all(st > 0 for t in (pred, real) for size, st in zip(t.shape, t.stride()) if size > 1))

        def _native_eval_iters(self, data, scaler, loader=None):
            """base_tsf_runner.py:257-273 with the rescaling and the three metrics in one ``EvalMetrics.update``, nothing read back"""
            mean, std = scaler
            forward_return = self.forward(data=data, epoch=None, iter_num=None, train=False)
            pred, real = forward_return[0], forward_return[1]
            ok = self._qualifies(pred, real) and self._scaler_fits(scaler, pred)
            if not ok and self._spread_acting:
                raise RuntimeError("step_amd.runner: a validation forward whose outputs EvalMetrics cannot take, in a pass spread over the "
                                   "ranks (spread_eval): the torch path would leave the other ranks waiting in the pass's collective")
            if not ok:
                # the forward pass is done and cannot be repeated: the base class's tail (:267-273) on torch ops, the scaler being
                # re_standard_transform (basicts/data/transform.py:59-65)
                prediction_rescaled, real_value_rescaled = self._rescaled(pred, mean, std), self._rescaled(real, mean, std)
                for metric_name, metric_func in self.metrics.items():
                    metric_item = self.metric_forward(metric_func, [prediction_rescaled, real_value_rescaled])
                    self.update_epoch_meter("val_" + metric_name, metric_item.item())
                return
            loader = getattr(self, "val_data_loader", None) if loader is None else loader
            group = loader.group_size if isinstance(loader, LookaheadLoader) and loader.coalesce > 1 else None
            self._val_accumulator(pred.shape[1], mean, std, pred.device).update(pred, real, group=group)

        # ---------------------------------------------------------------- TSFormer pre-training (native_pretrain=True)
        def _pretrain_scaler(self, data):
            """(mean, std) when everything known BEFORE the forward pass allows ``TSFormer.pretrain_tail``, else None"""
            if self._pretrain_module() is None or getattr(self, "cl_param", None):
                return None
            if not (isinstance(data, (tuple, list)) and len(data) == 2):          # (future_data, history_data), tsformer_runner.py:57
                return None
            if not str(getattr(self.loss, "__module__", "")).startswith(("basicts.", "step_amd.")):
                return None
            scaler = self._scalar_rescale(("masked_mae", "masked_mae_native"))
            # (a per-node scaler: the reference's broadcast against the pre-training [B, L', N] does not mean "per node" -- the base path)
            return None if scaler is None or isinstance(scaler[0], np.ndarray) else scaler

        def _pretrain_tail(self, data, scaler):
            """tsformer_runner.py:57-65 and base_tsf_runner.py:240-254 (:266-273 in validation) from one pretrain_tail call"""
            history_data = self.select_input_features(self.to_running_device(data[1]))
            nv = float(self.null_val)
            return self.model.pretrain_tail(history_data, null_val=None if nv != nv else nv, rescale=scaler)          # (None: the NaN rule)

        def val_iters(self, iter_index, data):
            scaler = self._pretrain_scaler(data) if native_pretrain else None
            if scaler is None:
                scaler = self._eval_scaler()
                if scaler is not None:
                    return self._native_eval_iters(data, scaler)
                return super().val_iters(iter_index, data)
            with torch.no_grad():
                _, three = self._pretrain_tail(data, scaler)
            for metric_name, metric_func in self.metrics.items():          # fed with the other deferred values when the epoch's meters are printed
                self.update_epoch_meter("val_" + metric_name, _Deferred(three[self._NATIVE_METRICS[metric_func.__name__]]))

        def test(self, *args, **kwargs):
            """``TSFormerRunner.test`` (step/step_runner/tsformer_runner.py:73-90) under ``native_pretrain``: one ``pretrain_tail`` call per
            batch, the three ``test_`` meters queued on the device like the validation ones.  A forecasting runner's ``test()`` under
            ``native_test``: ``_native_test`` (one ``EvalMetrics`` per pass).  Every other runner's ``test()`` is its own"""
            if self._pretrain_module() is None:
                scaler = self._eval_conditions() if native_test else None
                if scaler is None:
                    self._per_node_without_native_test()
                    return super().test(*args, **kwargs)
                if self._rank_world()[0] != 0:
                    return None          # (the reference's test() is master_only; the other ranks of a spread pass: _helper_passes)
                return self._native_test(scaler, self.test_data_loader, lambda: super(NativeRunner, self).test(*args, **kwargs))
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
                return None          # (the reference's test() is master_only)
            batches = iter(self.test_data_loader)
            data = next(batches, None)
            scaler = None if data is None else self._pretrain_scaler(data)          # (the batch form: a loader's batches all have one)
            if scaler is None:
                del batches
                return super().test(*args, **kwargs)
            with torch.no_grad():
                while data is not None:
                    _, three = self._pretrain_tail(data, scaler)
                    for metric_name, metric_func in self.metrics.items():
                        self.update_epoch_meter("test_" + metric_name, _Deferred(three[self._NATIVE_METRICS[metric_func.__name__]]))
                    data = next(batches, None)
            return None

        def _per_node_without_native_test(self):
            if test_per_node and not self._per_node_warned and self._rank_world()[0] == 0:
                import warnings
                self._per_node_warned = True
                warnings.warn("step_amd.runner: test_per_node needs native_test in effect (a STEP on a GPU, the re_standard_transform "
                              "scaler, only the three basicts metrics, a real null_val); the test pass has no per-sensor table")

        # ---------------------------------------------------------------- the forecasting test pass on the device (native_test=True)
        def _native_test(self, scaler, loader, base_test=None):
            """base_tsf_runner.py:277-318 from one ``EvalMetrics``: one accumulate launch per batch on the normalised prediction and the
            batch's target view, nothing kept, one read-back; then the reference's line per evaluation horizon and the three ``test_``
            meters from the overall row.  ``base_test``: what to run instead when the FIRST forward's outputs do not qualify (rank 0 of
            an unspread pass only; that batch is then forwarded twice).  On a rank other than 0 (a spread pass) nothing is logged"""
            from .evaluate import EvalMetrics
            mean, std = scaler
            rank = self._rank_world()[0]
            nodes = int(_unwrap(self.model).backend.num_nodes) if test_per_node else None
            m = None
            with torch.no_grad():
                for data in loader:
                    forward_return = self.forward(data, epoch=None, iter_num=None, train=False)
                    pred, real = forward_return[0], forward_return[1]
                    if not (self._qualifies(pred, real) and self._scaler_fits(scaler, pred)):
                        if m is None and base_test is not None and not self._spread_acting:
                            self._per_node_without_native_test()
                            return base_test()
                        raise RuntimeError("step_amd.runner: native_test met a forward whose outputs EvalMetrics cannot take "
                                           f"(prediction {tuple(getattr(pred, 'shape', ()))}, {getattr(pred, 'dtype', type(pred))})")
                    if m is None:
                        m = EvalMetrics(pred.shape[1], float(self.null_val), rescale=(std, mean), device=pred.device, nodes=nodes)
                    m.update(pred, real)
            if self._spread_acting:
                if m is None and loader.total_batches() > 0:          # a rank without a batch of its own still answers the collective
                    H = int(getattr(loader.dataset, "future_len", 12))
                    m = EvalMetrics(H, float(self.null_val), rescale=(std, mean), device=next(_unwrap(self.model).parameters()).device,
                                    nodes=nodes)
                if m is not None:
                    m.all_reduce(_unwrap(self.model)._process_group)          # the pass's one collective
            if m is None or rank != 0:
                return None
            res = m.result()
            self.eval_readbacks += 1
            names = [(metric_name, self._NATIVE_METRICS[metric_func.__name__]) for metric_name, metric_func in self.metrics.items()]
            for i in self.evaluation_horizons:
                metric_repr = ""
                for metric_name, k in names:
                    metric_repr += ", Test {0}: {1:.4f}".format(metric_name, float(res.per_horizon[i][k]))
                log = "Evaluate best model on test data for horizon {:d}" + metric_repr
                self.logger.info(log.format(i + 1))
            if test_per_node:
                self.test_result = res
                mae = res.per_node_overall[:, 0]
                worst = sorted(range(len(mae)), key=lambda n: (-mae[n], n))[:5]
                self.logger.info("Test MAE per sensor over all horizons, the largest (sensor: MAE): "
                                 + ", ".join("{:d}: {:.4f}".format(n, float(mae[n])) for n in worst))
            for metric_name, k in names:
                super().update_epoch_meter("test_" + metric_name, float(res.overall[k]))
            return None

        # ---------------------------------------------------------------- a rank other than 0 in spread validation / test passes
        def _helper_passes(self, epoch):
            """this rank's share of the passes due at the end of ``epoch`` (the arithmetic of base_runner.py:143-148), in rank 0's order:
            validation, then test -- each ends in the pass's one collective"""
            model = _unwrap(self.model)
            scaler = self._eval_scaler()
            if scaler is None:
                raise RuntimeError("step_amd.runner: spread_eval is acting but native_eval is no longer usable on this rank")
            mean, std = scaler
            val, test = self._helper_loaders["val"], self._helper_loaders["test"]
            was_training = model.training
            model.eval()
            try:
                with torch.no_grad():
                    if epoch % int(getattr(self, "val_interval", 1)) == 0 and val.total_batches() > 0:
                        for data in val:
                            self._native_eval_iters(data, scaler, loader=val)
                        dev = next(model.parameters()).device
                        m = self._val_accumulator(int(getattr(val.dataset, "future_len", 12)), mean, std, dev)
                        m.all_reduce(model._process_group)
                        m.reset()          # (the table is rank 0's to read)
                    if epoch % int(getattr(self, "test_interval", 1)) == 0:
                        self._native_test(scaler, test)
            finally:
                model.train(was_training)

        def _native_tail_iters(self, epoch, iter_index, data, scaler):
            """base_tsf_runner.py:237-255 with the rescaling, the curriculum slice, the loss and the three metrics in one train_tail call"""
            from .step_loss import train_tail
            mean, std = scaler
            iter_num = (epoch - 1) * self.iter_per_epoch + iter_index
            forward_return = list(self.forward(data=data, epoch=epoch, iter_num=iter_num, train=True))
            cl = self.curriculum_learning(epoch=epoch) if getattr(self, "cl_param", None) else None
            ok = len(forward_return) == 5
            if ok:
                pred, real, theta, prior, coef = forward_return
                ok = (torch.is_tensor(pred) and torch.is_tensor(real) and pred.is_cuda and real.is_cuda and pred.dtype == torch.float32
                      and real.dtype == torch.float32 and pred.dim() == 4 and pred.shape[3] == 1 and pred.shape == real.shape
                      and pred.shape[1] <= 64 and torch.is_tensor(theta) and theta.is_cuda and theta.dtype == torch.float32
                      and torch.is_tensor(prior) and not torch.is_tensor(coef) and (cl is None or 1 <= cl <= pred.shape[1])
                      and self._scaler_fits(scaler, pred))
            if not ok:
                # the forward pass is done and cannot be repeated: the base class's tail (:240-254) on torch ops, the scaler being
                # re_standard_transform (basicts/data/transform.py:59-65)
                forward_return[0] = self._rescaled(forward_return[0], mean, std)
                forward_return[1] = self._rescaled(forward_return[1], mean, std)
                if cl is not None:
                    forward_return[0] = forward_return[0][:, :cl, :, :]
                    forward_return[1] = forward_return[1][:, :cl, :, :]
                loss = self.metric_forward(self.loss, forward_return)
                for metric_name, metric_func in self.metrics.items():
                    metric_item = self.metric_forward(metric_func, forward_return[:2])
                    self.update_epoch_meter("train_" + metric_name, metric_item.item())
                return loss
            loss, three = train_tail(pred, real, theta, prior, coef, null_val=float(self.null_val), rescale=(mean, std), horizons=cl)
            for metric_name, metric_func in self.metrics.items():
                self.update_epoch_meter("train_" + metric_name, _Deferred(three[self._NATIVE_METRICS[metric_func.__name__]]))
            return loss

        def metric_forward(self, metric_func, args):
            if self._deferring and metric_func is not self.loss and native_metrics:
                # the three metrics of basicts/metrics the runner evaluates per iteration (base_tsf_runner.py:252-254), from one launch
                k = self._NATIVE_METRICS.get(getattr(metric_func, "__name__", None))
                nv = getattr(self, "null_val", 0.0)
                if (k is not None and str(getattr(metric_func, "__module__", "")).startswith("basicts.metrics") and len(args) == 2
                        and torch.is_tensor(args[0]) and args[0].is_cuda and args[0].dtype == torch.float32 and torch.is_tensor(args[1])
                        and args[1].dtype == torch.float32 and args[0].shape == args[1].shape and nv == nv):
                    c = self._metric_cache
                    if c is None or c[0] is not args[0] or c[1] is not args[1]:
                        from .step_loss import masked_metrics_native
                        c = self._metric_cache = (args[0], args[1], masked_metrics_native(args[0], args[1], float(nv)))
                    return _Deferred(c[2][k])
            out = super().metric_forward(metric_func, args)
            if self._deferring and metric_func is not self.loss and torch.is_tensor(out) and out.is_cuda:
                return _Deferred(out.detach())
            return out

        def update_epoch_meter(self, name, value, n=1):
            if isinstance(value, _Deferred):
                self._pending.setdefault(name, []).append((value.value, n))          # kept on the device: nothing is launched, nothing waited for
                return
            super().update_epoch_meter(name, value, n)

        def flush_meters(self):
            """feed the deferred values to the epoch meters (one device synchronisation for all of them), then what a ``native_eval``
            validation pass accumulated (its one read-back)"""
            pending, self._pending = self._pending, {}
            if pending:
                means, counts = [], []
                for name, items in pending.items():
                    vals = torch.stack([v.float().reshape(()) for v, _ in items])
                    ns = torch.tensor([float(n) for _, n in items], device=vals.device)
                    means.append((vals * ns).sum() / ns.sum())
                    counts.append(sum(n for _, n in items))
                for name, m, c in zip(pending, torch.stack(means).cpu().tolist(), counts):
                    super().update_epoch_meter(name, m, c)
            self._drain_val_metrics()

        def print_epoch_meters(self, meter_type):
            self.flush_meters()
            return super().print_epoch_meters(meter_type)

        def plt_epoch_meters(self, meter_type, step):
            self.flush_meters()
            return super().plt_epoch_meters(meter_type, step)

        def on_validating_end(self, *args, **kwargs):
            self.flush_meters()          # (base_tsf_runner.py:321-329 picks the best model by the epoch's val_MAE)
            return super().on_validating_end(*args, **kwargs)

        # ---------------------------------------------------------------- the epoch's end with the graph learner in time slices
        def _gather_slices(self):
            """ALL ranks: every rank's ``fc.weight`` slice into every rank's ``fc.weight`` (one gather of the matrix), then the two
            moments of the slices onto rank 0 (two more).  What follows on rank 0 alone -- the master-only validation, test and
            ``save_model`` -- then runs the whole graph learner without a collective and writes a complete checkpoint"""
            model = _unwrap(self.model)
            model.discrete_graph_learning.gather_fc_weight(model._process_group)
            self.optim.gather_state(model._process_group)

        def _with_gathered_slices(self, then, *args, **kwargs):
            if not self._shard_acting:
                return then(*args, **kwargs)
            self._gather_slices()
            try:
                return then(*args, **kwargs)
            finally:
                self.optim.release_state()

        if hasattr(base, "on_epoch_end"):
            def on_epoch_end(self, *args, **kwargs):
                """``basicts/runners/base_runner.py:132-152`` runs on every rank and calls the master-only ``validate``, ``test_process``
                and ``save_model``: the slices are gathered in front of it, the staging is released behind it"""
                return self._with_gathered_slices(self._epoch_end, *args, **kwargs)

            def _epoch_end(self, *args, **kwargs):
                if self._spread_acting:
                    epoch = int(args[0] if args else kwargs["epoch"])
                    if epoch % int(getattr(self, "val_interval", 1)) == 0 or epoch % int(getattr(self, "test_interval", 1)) == 0:
                        # every rank evaluates under rank 0's BatchNorm running statistics, as the master-only passes do (the ranks'
                        # own drift apart with their batches): one small broadcast per epoch's end, in front of the passes
                        from .comm import broadcast_running_statistics
                        model = _unwrap(self.model)
                        broadcast_running_statistics(model, model._process_group)
                        if self._rank_world()[0] != 0:
                            model._drop_eval_g()          # (a kept global feature was computed under the statistics just replaced)
                            # (the base class's validate / test_process / save_model are master-only: nothing of them runs here)
                            self._helper_passes(epoch)
                return super().on_epoch_end(*args, **kwargs)
        elif hasattr(base, "save_model"):
            def save_model(self, *args, **kwargs):
                """a base without ``on_epoch_end``: the same in front of ``save_model``, which every rank has to call"""
                return self._with_gathered_slices(super().save_model, *args, **kwargs)

    NativeRunner.__name__ = "Native" + base.__name__
    NativeRunner.__qualname__ = NativeRunner.__name__
    return NativeRunner
