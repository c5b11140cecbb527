"""``RunnerDouble`` with the validation side of the reference's runner restated: ``val_iters``
(``basicts/runners/base_tsf_runner.py:257-273``) and the ORDER of easytorch's ``validate`` (``model.eval()``, ``val_iters`` over
``self.val_data_loader``, ``print_epoch_meters("val")``, ``on_validating_end``), around the hooks ``step_amd.runner.native_runner``
overrides.  ``val_base_calls`` counts the batches that went through THIS class's ``val_iters``, ``meter_log`` holds every
``update_epoch_meter`` call that reached the base class as ``(name, value, n)``, ``predictions`` a clone of every forward's prediction."""
import torch

from tests.runner_double import RunnerDouble


class EvalRunnerDouble(RunnerDouble):
    """cfg as ``RunnerDouble``'s, plus "val_loader" / "test_loader": what ``build_val_data_loader`` / ``build_test_data_loader`` return"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.val_base_calls = 0
        self.meter_log = []
        self.predictions = []
        self.val_data_loader = None
        self.val_mae_at_validating_end = None

    def build_val_data_loader(self, cfg):
        return cfg.get("val_loader")

    def build_test_data_loader(self, cfg):
        return cfg.get("test_loader")

    def update_epoch_meter(self, name, value, n=1):
        self.meter_log.append((name, float(value), n))
        super().update_epoch_meter(name, value, n)

    def reset_epoch_meters(self):
        self.meters = {}

    def forward(self, data, epoch=None, iter_num=None, train=True, **kwargs):
        out = super().forward(data, epoch=epoch, iter_num=iter_num, train=train, **kwargs)
        self.predictions.append(out[0].detach().clone())
        return out

    # ---- base_tsf_runner.py:257-273
    def val_iters(self, iter_index, data):
        self.val_base_calls += 1
        forward_return = self.forward(data=data, epoch=None, iter_num=None, train=False)
        mean, std = self.scaler["args"]["mean"], self.scaler["args"]["std"]
        prediction_rescaled = forward_return[0] * std + mean          # re_standard_transform, basicts/data/transform.py:59-65
        real_value_rescaled = forward_return[1] * std + mean
        for metric_name, metric_func in self.metrics.items():
            metric_item = self.metric_forward(metric_func, [prediction_rescaled, real_value_rescaled])
            self.update_epoch_meter("val_" + metric_name, metric_item.item())

    # ---- base_tsf_runner.py:321-329 reads the epoch's val_MAE here (save_best_model)
    def on_validating_end(self, train_epoch=None):
        m = self.meters.get("val_MAE")
        self.val_mae_at_validating_end = None if m is None else m.avg

    # ---- the order of easytorch's Runner.validate
    @torch.no_grad()
    def validate(self, train_epoch=None):
        self.model.eval()
        for iter_index, data in enumerate(self.val_data_loader):
            self.val_iters(iter_index, data)
        self.print_epoch_meters("val")
        self.on_validating_end(train_epoch)
