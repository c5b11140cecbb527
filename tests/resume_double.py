"""easytorch's checkpoint protocol on top of ``RunnerDouble``, for tests that resume a run and have no easytorch at hand.

RESTATED FROM MEMORY of easy-torch 1.2.10 (``easytorch/core/runner.py``: ``init_training``, ``save_model``, ``load_model_resume``; the
package is not installed where these tests were written) and from the finding in ADVICE.md that describes it: ``init_training`` builds
the optimizer and the scheduler from ``CFG.TRAIN`` and THEN calls ``load_model_resume()``, which loads the newest checkpoint of the
run's directory, restores model, optimizer, ``start_epoch`` and ``best_metrics``, sets ``scheduler.last_epoch`` (nothing else of the
scheduler is saved) and swallows ``(IndexError, OSError, KeyError)`` -- no checkpoint yet, or one it cannot read.  A checkpoint is the
dict ``{"epoch", "model_state_dict", "optim_state_dict", "best_metrics"}`` written with ``torch.save``.

cfg (besides RunnerDouble's): ``"ckpt_dir"`` (the run's checkpoint directory) and ``"all_params"`` (True: Adam is given
``model.parameters()``, as easytorch does; False: only the trainable ones, as tests/_shims/easytorch does)."""
import glob
import os

import torch

from tests.runner_double import RunnerDouble


class ResumeProtocol:
    """the three methods, for any RunnerDouble (``class X(ResumeProtocol, SomeRunnerDouble)``)"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.ckpt_save_dir = cfg["ckpt_dir"]
        self.all_params = cfg.get("all_params", True)
        self.start_epoch = 0
        self.best_metrics = {}
        self.optim = self.scheduler = self.clip_grad_param = None
        self.resume_errors = []          # what load_model_resume swallowed
        self.scheduler_after_resume = None

    def init_training(self, cfg):
        params = list(self.model.parameters())
        if not self.all_params:
            params = [p for p in params if p.requires_grad]
        self.optim = torch.optim.Adam(params, **cfg["TRAIN"]["OPTIM"]["PARAM"])
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optim, **cfg["TRAIN"]["LR_SCHEDULER"]["PARAM"])
        self.clip_grad_param = dict(cfg["TRAIN"]["CLIP_GRAD_PARAM"])
        self.load_model_resume()
        self.scheduler_after_resume = dict(self.scheduler.state_dict())          # what the protocol left on the scheduler it built

    def save_model(self, epoch):
        os.makedirs(self.ckpt_save_dir, exist_ok=True)
        ckpt = {"epoch": epoch, "model_state_dict": self.model.state_dict(), "optim_state_dict": self.optim.state_dict(),
                "best_metrics": self.best_metrics}
        path = os.path.join(self.ckpt_save_dir, "ckpt_{:03d}.pt".format(epoch))
        torch.save(ckpt, path)
        return path

    def load_model_resume(self, strict=True):
        try:
            path = sorted(glob.glob(os.path.join(self.ckpt_save_dir, "ckpt_*.pt")))[-1]
            ckpt = torch.load(path, map_location=next(self.model.parameters()).device)
            self.model.load_state_dict(ckpt["model_state_dict"], strict=strict)
            self.optim.load_state_dict(ckpt["optim_state_dict"])
            self.start_epoch = ckpt["epoch"]
            if ckpt.get("best_metrics") is not None:
                self.best_metrics = ckpt["best_metrics"]
            if self.scheduler is not None:
                self.scheduler.last_epoch = ckpt["epoch"]
        except (IndexError, OSError, KeyError) as e:
            self.resume_errors.append(e)

    # ---- easytorch's epoch loop around train_iters (Runner.train / backward / on_epoch_end), one epoch of it
    def train_epoch(self, epoch, batches, before_iteration=None):
        self.model.train()
        for it, batch in enumerate(batches):
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


class ResumeRunnerDouble(ResumeProtocol, RunnerDouble):
    """RunnerDouble (the STEP runner's forward and training iteration) with the checkpoint protocol"""
