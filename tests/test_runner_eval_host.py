"""Host side of the runner's validation / test passes (no GPU): ``coalesce_origin_batches``, the length and the factor of a coalescing
``LookaheadLoader``, the defaults of the two switches, and ``native_eval=True`` around a model that is not a ``STEP`` on a GPU (the base
class's ``val_iters`` is what runs).  On the device: tests/test_gpu_runner_eval.py."""
import inspect

import pytest
import torch

from tests.eval_runner_double import EvalRunnerDouble
from tests.runner_double import masked_mae


def _origin_batches():
    return [torch.tensor(b, dtype=torch.int64) for b in ([300, 288], [350, 310], [100, 388], [295, 377], [333])]


def test_coalesce_origin_batches():
    from step_amd.runner import coalesce_origin_batches
    batches = _origin_batches()
    flat = torch.cat(batches)
    by_two = list(coalesce_origin_batches(iter(batches), 2))
    assert [b.tolist() for b in by_two] == [[300, 288, 350, 310], [100, 388, 295, 377], [333]]
    assert all(b.dtype == torch.int64 and b.dim() == 1 for b in by_two)
    same = list(coalesce_origin_batches(batches, 1))
    assert len(same) == 5 and all(x is y for x, y in zip(same, batches))          # k = 1: the very objects
    one = list(coalesce_origin_batches(batches, 5))
    assert len(one) == 1 and torch.equal(one[0], flat)
    more = list(coalesce_origin_batches(batches, 7))
    assert len(more) == 1 and torch.equal(more[0], flat)
    by_three = list(coalesce_origin_batches(batches, 3))
    assert [b.tolist() for b in by_three] == [[300, 288, 350, 310, 100, 388], [295, 377, 333]]
    assert list(coalesce_origin_batches([], 2)) == [] and list(coalesce_origin_batches(iter(()), 1)) == []
    with pytest.raises(ValueError):
        list(coalesce_origin_batches(batches, 0))


class _Origins(torch.utils.data.Dataset):
    index_only = True

    def __init__(self, origins, index_only=True):
        self.origins, self.index_only = origins, index_only

    def __getitem__(self, i):
        return torch.tensor(self.origins[i], dtype=torch.int64)

    def __len__(self):
        return len(self.origins)


def _loader(batch_size=2, index_only=True):
    return torch.utils.data.DataLoader(_Origins([300, 288, 350, 310, 100, 388, 295, 377, 333], index_only), batch_size=batch_size, shuffle=False)


def test_lookahead_loader_length_and_group_size_under_coalescing():
    from step_amd.runner import LookaheadLoader
    loader = _loader()
    assert len(loader) == 5
    for k, want in ((1, 5), (2, 3), (3, 2), (4, 2), (5, 1), (9, 1)):
        look = LookaheadLoader(loader, None, prefetch=False, coalesce=k)
        assert len(look) == want and look.coalesce == k and look.group_size == 2 and look.batch_size == 2
    assert LookaheadLoader(loader, None).coalesce == 1          # the default: as before
    with pytest.raises(ValueError):
        LookaheadLoader(loader, None, coalesce=0)
    with pytest.raises(ValueError):
        LookaheadLoader(_loader(index_only=False), None, coalesce=2)          # host windows are not concatenated


class _CpuModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.5))

    def forward(self, history_data, long_history_data, future_data, batch_seen, epoch):
        return history_data[..., :1] * self.w, None, None, None


def _runner(val_loader=None, model=None, **switches):
    from step_amd.runner import native_runner
    cfg = {"model": model or _CpuModel(), "loss": masked_mae, "scaler": (3.25, 1.75), "cl": None, "val_loader": val_loader}
    runner = native_runner(EvalRunnerDouble, **switches)(cfg)
    runner.val_data_loader = runner.build_val_data_loader(cfg)
    return runner, cfg


@pytest.mark.parametrize("E, k", [(1, 1), (5, 2), (8, 4)])
def test_coalesce_factor_of_the_eval_loaders(E, k):
    from step_amd.runner import LookaheadLoader
    runner, cfg = _runner(_loader(), eval_batch_size=E)
    assert isinstance(runner.val_data_loader, LookaheadLoader) and runner.val_data_loader.coalesce == k == max(1, E // 2)
    assert runner.val_data_loader.prefetch is False and len(runner.val_data_loader) == -(-5 // k)
    cfg["test_loader"] = _loader()
    assert runner.build_test_data_loader(cfg).coalesce == k


def test_eval_batch_size_is_ignored_where_it_cannot_apply():
    from step_amd.runner import coalesce_factor
    assert _runner(_loader())[0].val_data_loader.coalesce == 1                                   # the default: None
    assert _runner(_loader(index_only=False), eval_batch_size=8)[0].val_data_loader.coalesce == 1          # not origins
    assert _runner(_loader(batch_size=None), eval_batch_size=8)[0].val_data_loader.coalesce == 1           # no integer batch size
    assert _runner(None, eval_batch_size=8)[0].val_data_loader is None
    assert coalesce_factor(64, _loader(batch_size=8)) == 8 and coalesce_factor(None, _loader()) == 1


def test_the_switches_default_to_off():
    from step_amd.runner import native_runner
    sig = inspect.signature(native_runner)
    assert sig.parameters["native_eval"].default is False and sig.parameters["eval_batch_size"].default is None


class _WithTest(EvalRunnerDouble):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.test_base_calls = 0

    def test(self):
        self.test_base_calls += 1
        return "base"


@pytest.mark.parametrize("native_pretrain", (False, True))
def test_test_reaches_the_base_class_without_a_pretraining_module_on_a_gpu(native_pretrain):
    from step_amd.runner import native_runner
    runner = native_runner(_WithTest, native_pretrain=native_pretrain)({"model": _CpuModel(), "loss": masked_mae, "scaler": (3.25, 1.75), "cl": None})
    assert runner.test() == "base" and runner.test_base_calls == 1 and runner._pending == {}


@pytest.mark.parametrize("native_eval", (False, True))
def test_a_cpu_model_keeps_the_base_val_iters(native_eval):
    runner, _ = _runner(model=_CpuModel(), native_eval=native_eval)
    gen = torch.Generator().manual_seed(3)
    fut, hist, long_hist = torch.randn(2, 12, 5, 3, generator=gen), torch.randn(2, 12, 5, 3, generator=gen), torch.randn(2, 24, 5, 3, generator=gen)
    runner.val_data_loader = [(fut, hist, long_hist)]
    runner.validate()
    assert runner.val_base_calls == 1 and runner._val_metrics is None
    assert [(name, n) for name, _v, n in runner.meter_log] == [("val_MAE", 1), ("val_RMSE", 1), ("val_MAPE", 1)]
    want = masked_mae(hist[..., :1] * 0.5 * 1.75 + 3.25, fut[..., :1] * 1.75 + 3.25)
    assert runner.meters["val_MAE"].avg == pytest.approx(float(want), rel=1e-6)
    assert runner.val_mae_at_validating_end == runner.meters["val_MAE"].avg
