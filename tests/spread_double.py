"""Doubles for the tests of ``native_runner(..., native_test=True)`` and ``spread_eval=True`` that have no reference checkout at hand.

``TestPassDouble``: ``EvalRunnerDouble`` (the validation side) plus the forecasting ``test()`` RESTATED in the project's own words from
what ``basicts/runners/base_tsf_runner.py:277-318`` does -- master-only, under ``no_grad``: every batch's prediction and label kept,
concatenated, rescaled; per evaluation horizon the three metrics on that horizon's slice, logged in one line; the three metrics on
everything to the ``test_`` meters.  ``logger.lines`` holds what was logged, ``test_base_calls`` counts the passes through THIS ``test()``.

``SpreadRunnerDouble``: that on top of easytorch's distributed protocol (tests/dp_double.py) with the end of an epoch restated from
``basicts/runners/base_runner.py``: ``init_training`` builds the validation and test loaders on rank 0 only (``init_validation`` /
``init_test`` are master-only); ``on_epoch_end(epoch)`` runs on EVERY rank -- train meters, then the master-only ``validate`` (every
``val_interval`` epochs; the order of tests/eval_runner_double.py) and ``test_process`` (every ``test_interval`` epochs: eval mode,
``test()``, the test meters), ``save_model``, and the meters are reset.  ``epoch_meters[epoch]`` keeps the averages of every meter as
they stood before the reset; ``eval_forwards`` counts the forwards with ``train=False`` and ``eval_batches`` keeps their origins.  Both
master-only passes put the model back in train mode, as the next epoch's start does in easytorch."""
import torch
import torch.distributed as dist

from tests.dp_double import DistributedProtocol, _distributed
from tests.eval_runner_double import EvalRunnerDouble


def _master():
    return not _distributed() or dist.get_rank() == 0


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line)


class TestPassDouble(EvalRunnerDouble):
    __test__ = False          # (not a test class, whatever its name starts with)

    def __init__(self, cfg):
        super().__init__(cfg)
        self.evaluation_horizons = range(12)
        self.evaluate_on_gpu = True
        self.logger = _Log()
        self.test_data_loader = None
        self.test_base_calls = 0
        self.eval_forwards = 0
        self.eval_batches = []          # the host origins of every batch forwarded with train=False (index-only batches)

    def forward(self, data, epoch=None, iter_num=None, train=True, **kwargs):
        if not train:
            self.eval_forwards += 1
            self.eval_batches.append(getattr(data[2], "t0_host", None))
        return super().forward(data, epoch=epoch, iter_num=iter_num, train=train, **kwargs)

    @torch.no_grad()
    def test(self):
        if not _master():
            return
        self.test_base_calls += 1
        prediction, real_value = [], []
        for _, data in enumerate(self.test_data_loader):
            forward_return = self.forward(data, epoch=None, iter_num=None, train=False)
            prediction.append(forward_return[0])
            real_value.append(forward_return[1])
        prediction, real_value = torch.cat(prediction, dim=0), torch.cat(real_value, dim=0)
        mean, std = self.scaler["args"]["mean"], self.scaler["args"]["std"]
        prediction, real_value = prediction * std + mean, real_value * std + mean
        for i in self.evaluation_horizons:
            pred, real = prediction[:, i, :, :], real_value[:, i, :, :]
            metric_repr = ""
            for metric_name, metric_func in self.metrics.items():
                metric_item = self.metric_forward(metric_func, [pred, real])
                metric_repr += ", Test {0}: {1:.4f}".format(metric_name, metric_item.item())
            log = "Evaluate best model on test data for horizon {:d}" + metric_repr
            self.logger.info(log.format(i + 1))
        for metric_name, metric_func in self.metrics.items():
            metric_item = self.metric_forward(metric_func, [prediction, real_value])
            self.update_epoch_meter("test_" + metric_name, metric_item.item())


class SpreadRunnerDouble(DistributedProtocol, TestPassDouble):
    """cfg (besides DistributedProtocol's and EvalRunnerDouble's): "val_interval", "test_interval" (default 1).  The dict handed to
    ``init_training`` carries "val_loader" / "test_loader" next to "TRAIN"."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.val_interval, self.test_interval = cfg.get("val_interval", 1), cfg.get("test_interval", 1)
        self.epoch_meters = {}

    def init_training(self, cfg):
        super().init_training(cfg)
        if _master():          # init_validation / init_test
            self.val_data_loader = self.build_val_data_loader(cfg)
            self.test_data_loader = self.build_test_data_loader(cfg)

    def validate(self, train_epoch=None):
        if not _master():
            return
        try:
            super().validate(train_epoch)
        finally:
            self.model.train()

    @torch.no_grad()
    def test_process(self, train_epoch=None):
        if not _master():
            return
        self.model.eval()
        try:
            self.test()
            self.print_epoch_meters("test")
        finally:
            self.model.train()

    def on_epoch_end(self, epoch):
        self.print_epoch_meters("train")
        self.plt_epoch_meters("train", epoch)
        if self.val_data_loader is not None and epoch % self.val_interval == 0:
            self.validate(train_epoch=epoch)
        if self.test_data_loader is not None and epoch % self.test_interval == 0:
            self.test_process(train_epoch=epoch)
        path = self.save_model(epoch)
        self.epoch_meters[epoch] = {k: m.avg for k, m in self.meters.items()}
        self.reset_epoch_meters()
        return path

    def train_loader_epoch(self, epoch, before_iteration=None, seen=None):
        loader = self.train_data_loader
        if _distributed():
            loader.sampler.set_epoch(epoch)
        self.model.train()
        for it, batch in enumerate(loader):
            if seen is not None:
                seen.append(batch)
            if before_iteration is not None:
                before_iteration(epoch, it)
            loss = self.train_iters(epoch, it, batch)
            self.optim.zero_grad()
            loss.backward()
            if self.clip_grad_param is not None:
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), **self.clip_grad_param)
            self.optim.step()
        self.scheduler.step()
        return self.on_epoch_end(epoch)
