"""A stand-in for the reference's runner base classes in tests that have no reference checkout at hand: the training iteration of
``basicts/runners/base_tsf_runner.py:170-255`` (``curriculum_learning``, ``metric_forward``, ``train_iters`` and its meter calls) and
``STEPRunner.forward`` (``step/step_runner/step_runner.py:43-75``) restated, around the hooks ``step_amd.runner.native_runner``
overrides.  ``base_calls`` counts the iterations that went through THIS class's ``train_iters``."""
import torch


def _mask_of(labels, null_val):
    m = (~torch.isclose(labels, torch.tensor(null_val).expand_as(labels).to(labels.device), atol=5e-5, rtol=0.)).float()
    m = m / torch.mean(m)
    return torch.where(torch.isnan(m), torch.zeros_like(m), m)


def masked_mae(preds, labels, null_val=0.0):
    loss = torch.abs(preds - labels) * _mask_of(labels, null_val)
    return torch.mean(torch.where(torch.isnan(loss), torch.zeros_like(loss), loss))


def masked_rmse(preds, labels, null_val=0.0):
    loss = (preds - labels) ** 2 * _mask_of(labels, null_val)
    return torch.sqrt(torch.mean(torch.where(torch.isnan(loss), torch.zeros_like(loss), loss)))


def masked_mape(preds, labels, null_val=0.0):
    labels = torch.where(torch.abs(labels) < 1e-4, torch.zeros_like(labels), labels)
    loss = torch.abs(torch.abs(preds - labels) / labels) * _mask_of(labels, 0.0)
    return torch.mean(torch.where(torch.isnan(loss), torch.zeros_like(loss), loss))


# the runner recognises the three metrics of basicts/metrics by name and module (step_amd/runner.py, metric_forward)
masked_mae.__module__, masked_rmse.__module__, masked_mape.__module__ = "basicts.metrics.mae", "basicts.metrics.rmse", "basicts.metrics.mape"


class Meter:
    def __init__(self):
        self.sum, self.n = 0.0, 0

    @property
    def avg(self):
        return self.sum / self.n if self.n else 0.0


class RunnerDouble:
    """cfg: {"model", "loss", "scaler": (mean, std), "cl": None | {"WARM_EPOCHS", "CL_EPOCHS", "PREDICTION_LENGTH", "STEP_SIZE"},
    "iter_per_epoch"}"""

    def __init__(self, cfg):
        self.model = cfg["model"]
        self.loss = cfg["loss"]
        self.metrics = {"MAE": masked_mae, "RMSE": masked_rmse, "MAPE": masked_mape}
        mean, std = cfg["scaler"]
        self.scaler = {"func": "re_standard_transform", "args": {"mean": mean, "std": std}}
        self.null_val = 0.0
        self.forward_features = [0, 1, 2]
        self.target_features = [0]
        self.iter_per_epoch = cfg.get("iter_per_epoch", 10)
        self.cl_param = cfg.get("cl")
        if self.cl_param is not None:          # base_tsf_runner.py:45-50
            self.warm_up_epochs = self.cl_param.get("WARM_EPOCHS", 0)
            self.cl_epochs = self.cl_param.get("CL_EPOCHS")
            self.prediction_length = self.cl_param.get("PREDICTION_LENGTH")
            self.cl_step_size = self.cl_param.get("STEP_SIZE", 1)
        self.meters = {}
        self.base_calls = 0

    # ---- hooks native_runner() overrides and calls through super()
    def build_train_data_loader(self, cfg):
        return None

    def build_val_data_loader(self, cfg):
        return None

    def build_test_data_loader(self, cfg):
        return None

    def select_input_features(self, data):
        return data[:, :, :, self.forward_features]

    def select_target_features(self, data):
        return data[:, :, :, self.target_features]

    def init_training(self, cfg):
        pass

    def print_epoch_meters(self, meter_type):
        pass

    def plt_epoch_meters(self, meter_type, step):
        pass

    def update_epoch_meter(self, name, value, n=1):
        m = self.meters.setdefault(name, Meter())
        m.sum += float(value) * n
        m.n += n

    def to_running_device(self, t):
        return t.to(next(self.model.parameters()).device) if torch.is_tensor(t) else t

    # ---- step_runner.py:43-75
    def forward(self, data, epoch=None, iter_num=None, train=True, **kwargs):
        future_data, history_data, long_history_data = data
        history_data = self.to_running_device(history_data)
        long_history_data = self.to_running_device(long_history_data)
        future_data = self.to_running_device(future_data)
        history_data = self.select_input_features(history_data)
        long_history_data = self.select_input_features(long_history_data)
        prediction, pred_adj, prior_adj, gsl_coefficient = self.model(history_data=history_data, long_history_data=long_history_data,
                                                                      future_data=None, batch_seen=iter_num, epoch=epoch)
        batch_size, length, num_nodes, _ = future_data.shape
        assert list(prediction.shape)[:3] == [batch_size, length, num_nodes]
        prediction = self.select_target_features(prediction)
        real_value = self.select_target_features(future_data)
        return prediction, real_value, pred_adj, prior_adj, gsl_coefficient

    # ---- base_tsf_runner.py:170-190
    def curriculum_learning(self, epoch=None):
        if epoch is None:
            return self.prediction_length
        epoch -= 1
        if epoch < self.warm_up_epochs:
            cl_length = self.prediction_length
        else:
            _ = ((epoch - self.warm_up_epochs) // self.cl_epochs + 1) * self.cl_step_size
            cl_length = min(_, self.prediction_length)
        return cl_length

    # ---- base_tsf_runner.py:207-223
    def metric_forward(self, metric_func, args):
        return metric_func(*args, null_val=self.null_val)

    # ---- base_tsf_runner.py:225-255
    def train_iters(self, epoch, iter_index, data):
        self.base_calls += 1
        iter_num = (epoch - 1) * self.iter_per_epoch + iter_index
        forward_return = list(self.forward(data=data, epoch=epoch, iter_num=iter_num, train=True))
        mean, std = self.scaler["args"]["mean"], self.scaler["args"]["std"]
        prediction_rescaled = forward_return[0] * std + mean          # re_standard_transform, basicts/data/transform.py:59-65
        real_value_rescaled = forward_return[1] * std + mean
        if self.cl_param:
            cl_length = self.curriculum_learning(epoch=epoch)
            forward_return[0] = prediction_rescaled[:, :cl_length, :, :]
            forward_return[1] = real_value_rescaled[:, :cl_length, :, :]
        else:
            forward_return[0] = prediction_rescaled
            forward_return[1] = real_value_rescaled
        loss = self.metric_forward(self.loss, forward_return)
        for metric_name, metric_func in self.metrics.items():
            metric_item = self.metric_forward(metric_func, forward_return[:2])
            self.update_epoch_meter("train_" + metric_name, metric_item.item())
        return loss
