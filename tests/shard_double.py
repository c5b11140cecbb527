"""The end of an epoch on top of easytorch's distributed protocol (tests/dp_double.py), for tests of ``native_runner(...,
shard_graph_learner=True)`` that have no reference checkout at hand.

RESTATED in the project's own words from what ``basicts/runners/base_runner.py`` does when an epoch ends: ``on_epoch_end(epoch)`` is
called on EVERY rank; inside it the validation pass and ``save_model`` are master-only -- rank 0 runs an eval-mode forward under
``no_grad`` while the other ranks are already past it, then rank 0 writes the checkpoint.  The epoch loop of
``DistributedProtocol.train_loader_epoch`` ends in ``save_model`` itself; here it ends in ``on_epoch_end``.

cfg (besides DistributedProtocol's): ``"val_batch"`` -- one staged batch ``(future, history, long history)`` for the validation
forward (None: no validation).  ``validated`` collects ``(epoch, prediction)`` on the rank that validated."""
import torch
import torch.distributed as dist

from tests.dp_double import DistributedRunnerDouble, _distributed


class ShardRunnerDouble(DistributedRunnerDouble):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.val_batch = cfg.get("val_batch")
        self.validated = []

    def validate(self, epoch):
        if _distributed() and dist.get_rank() != 0:          # @master_only
            return
        if self.val_batch is None:
            return
        self.model.eval()
        try:
            with torch.no_grad():
                prediction = self.forward(data=self.val_batch, epoch=None, iter_num=None, train=False)[0]
            self.validated.append((epoch, prediction.detach().clone()))
        finally:
            self.model.train()

    def on_epoch_end(self, epoch):
        self.validate(epoch)
        return self.save_model(epoch)

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
