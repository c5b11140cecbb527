"""easytorch's DISTRIBUTED protocol on top of the checkpoint protocol of tests/resume_double.py, for tests that launch two ranks and have
no easytorch at hand.

RESTATED FROM MEMORY of easy-torch 1.2.10 (``easytorch/core/runner.py``; the package is not installed where these tests were written):

* the runner builds the model and, when ``torch.distributed`` is initialised, wraps it in ``DistributedDataParallel`` (``device_ids`` =
  the local device) before anything else sees it;
* ``init_training`` builds the training loader -- with a ``DistributedSampler`` when distributed --, then the optimizer and the
  scheduler, then calls ``load_model_resume()``;
* ``save_model`` runs on rank 0 only and stores ``model.module.state_dict()`` when the model is wrapped, so checkpoints never carry the
  ``module.`` prefix; ``load_model_resume`` loads into ``.module`` when wrapped;
* the epoch loop calls ``train_data_loader.sampler.set_epoch(epoch)`` when distributed, before it iterates.

cfg (besides ResumeProtocol's): ``"dataset"`` and ``"batch_size"`` of the training loader.  ``set_epoch_calls`` records the epochs the
sampler was told, read back FROM THE SAMPLER the loop reached through ``train_data_loader.sampler`` -- under ``native_runner`` that is
a ``LookaheadLoader``, which has to forward the attribute."""
import glob
import os

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

from tests.resume_double import ResumeProtocol
from tests.runner_double import RunnerDouble
from tests.test_gpu_pretrain_tail import PretrainRunnerDouble


def _distributed():
    return dist.is_available() and dist.is_initialized()


class RecordingSampler(DistributedSampler):
    """DistributedSampler that remembers what ``set_epoch`` was told"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.epochs_set = []

    def set_epoch(self, epoch):
        self.epochs_set.append(epoch)
        super().set_epoch(epoch)


class DistributedProtocol(ResumeProtocol):
    def __init__(self, cfg):
        super().__init__(cfg)
        self._dataset, self._batch_size = cfg.get("dataset"), cfg.get("batch_size", 2)
        self.train_data_loader = None
        if _distributed():
            p = next(self.model.parameters())
            self.model = DistributedDataParallel(self.model, device_ids=[p.device.index] if p.is_cuda else None)

    # ---- what native_runner's build_train_data_loader wraps
    def build_train_data_loader(self, cfg):
        if self._dataset is None:
            return None
        sampler = RecordingSampler(self._dataset, shuffle=True, seed=0) if _distributed() else None
        return DataLoader(self._dataset, batch_size=self._batch_size, sampler=sampler, shuffle=sampler is None)

    def init_training(self, cfg):
        self.train_data_loader = self.build_train_data_loader(cfg)
        super().init_training(cfg)          # optimizer, scheduler, load_model_resume()

    def _bare(self):
        return self.model.module if isinstance(self.model, DistributedDataParallel) else self.model

    def save_model(self, epoch):
        if _distributed() and dist.get_rank() != 0:          # @master_only
            return None
        os.makedirs(self.ckpt_save_dir, exist_ok=True)
        ckpt = {"epoch": epoch, "model_state_dict": self._bare().state_dict(), "optim_state_dict": self.optim.state_dict(),
                "best_metrics": self.best_metrics}
        path = os.path.join(self.ckpt_save_dir, "ckpt_{:03d}.pt".format(epoch))
        torch.save(ckpt, path)
        return path

    def load_model_resume(self, strict=True):
        try:
            path = sorted(glob.glob(os.path.join(self.ckpt_save_dir, "ckpt_*.pt")))[-1]
            ckpt = torch.load(path, map_location=next(self.model.parameters()).device)
            self._bare().load_state_dict(ckpt["model_state_dict"], strict=strict)
            self.optim.load_state_dict(ckpt["optim_state_dict"])
            self.start_epoch = ckpt["epoch"]
            if ckpt.get("best_metrics") is not None:
                self.best_metrics = ckpt["best_metrics"]
            if self.scheduler is not None:
                self.scheduler.last_epoch = ckpt["epoch"]
        except (IndexError, OSError, KeyError) as e:
            self.resume_errors.append(e)

    # ---- Runner.train's epoch over the runner's own loader
    def train_loader_epoch(self, epoch, before_iteration=None, seen=None):
        """one epoch; ``seen``: a list that collects every batch handed to ``train_iters``"""
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
        return self.save_model(epoch)


class DistributedRunnerDouble(DistributedProtocol, RunnerDouble):
    """the STEP runner's forward and training iteration under the distributed protocol"""


class DistributedPretrainRunnerDouble(DistributedProtocol, PretrainRunnerDouble):
    """the TSFormer runner's forward under the distributed protocol"""
