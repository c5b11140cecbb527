"""Evaluation metrics on the device: step_eval_metrics_* (through step_amd.EvalMetrics) against the numbers the reference's own
masked_mae / masked_rmse / masked_mape gave for tests/golden/eval_metrics_cases.npz (tools/make_eval_metrics_golden.py), and
STEP.evaluate on the step_small golden model against the same loop written by hand.  Host-side rules: tests/test_eval_metrics_host.py.

Bounds.  Against the fixture: relative 1e-5 (absolute 1e-6 where the reference gives 0) -- the reference is an f32 mean over at most
10 800 elements, the kernel sums the same f32 terms in f64, and a float64 restatement agrees with the reference to about 1e-7
(tests/test_eval_metrics_host.py holds it to 1e-5 as well), so the bound is two orders above f32 rounding.  Between two ways of
accumulating the same elements: relative 1e-12 -- both are f64 sums of identical f32 terms (at most 420 per horizon in case (a)) that
differ in the order of the additions only, which moves an f64 sum by a few 1e-16 of its value per addition at the very most."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics_cases.npz")
CASES = ["a", "b", "c1", "c2"]
NULLS = {"zero": 0.0, "nan": float("nan")}


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """device tensors of one case, uploaded once and left unchanged: prediction [B, H, N], the label tensor [B, H, N, C], its channel"""
    z = _fixture()
    return torch.from_numpy(z[f"{name}.pred"]).cuda(), torch.from_numpy(z[f"{name}.real"]).cuda(), int(z[f"{name}.channel"])


def _metrics(name, tag):
    from step_amd import EvalMetrics
    z = _fixture()
    return EvalMetrics(horizons=z[f"{name}.pred"].shape[1], null_val=NULLS[tag], rescale=(float(z[f"{name}.scale"]), float(z[f"{name}.shift"])))


def _assert_close(got, want, rel, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.where(want == 0.0, 1e-6, rel * np.abs(want))
    err = np.abs(got - want)
    print(f"{what}: largest |difference| / bound = {float(np.max(err / bound)):.3e}")
    assert got.shape == want.shape and np.all(err <= bound), (what, got, want)


def _feed(m, name, split):
    pred, real, c = _inputs(name)
    at = 0
    for n in split:
        m.update(pred[at:at + n], real[at:at + n, :, :, c])
        at += n
    assert at == pred.shape[0]
    return m.result()


# ---------------------------------------------------------------------------------------------- the kernel against the reference
@pytest.mark.parametrize("tag", sorted(NULLS))
@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_reference_metrics(name, tag):
    z = _fixture()
    B, H = z[f"{name}.pred"].shape[:2]
    one = _feed(_metrics(name, tag), name, [B])
    assert one.batches == 1 and one.per_horizon.shape == (H, 3) and one.per_horizon.dtype == np.float64 and one.horizons == tuple(range(H))
    _assert_close(one.per_horizon, z[f"{name}.{tag}.per_horizon"], 1e-5, f"{name}/{tag} per horizon")
    _assert_close(one.overall, z[f"{name}.{tag}.overall"], 1e-5, f"{name}/{tag} overall")
    _assert_close(one.batch_mean, z[f"{name}.{tag}.overall"], 1e-5, f"{name}/{tag} batch mean of one batch")
    split = z[f"{name}.split"].tolist()
    parts = _feed(_metrics(name, tag), name, split)
    assert parts.batches == len(split)
    _assert_close(parts.per_horizon, z[f"{name}.{tag}.per_horizon"], 1e-5, f"{name}/{tag} per horizon, split {split}")
    _assert_close(parts.overall, z[f"{name}.{tag}.overall"], 1e-5, f"{name}/{tag} overall, split {split}")
    _assert_close(parts.batch_mean, z[f"{name}.{tag}.batch_mean_split"], 1e-5, f"{name}/{tag} batch mean, split {split}")
    if name == "a" and tag == "zero":
        assert (one.per_horizon[4] == 0.0).all()          # the all-null horizon: a count of 0 gives exactly 0


def test_accumulation_over_batches_reset_and_repeated_result():
    z = _fixture()
    m = _metrics("a", "zero")
    one = _feed(m, "a", [7])
    again = m.result()
    for x, y in ((one.per_horizon, again.per_horizon), (one.overall, again.overall), (one.batch_mean, again.batch_mean)):
        assert np.array_equal(x, y)          # result() does not clear or change the accumulator
    m.reset()
    assert m.batches == 0
    parts = _feed(m, "a", [3, 3, 1])
    _assert_close(parts.per_horizon, one.per_horizon, 1e-12, "3 + 3 + 1 windows against one call, per horizon")
    _assert_close(parts.overall, one.overall, 1e-12, "3 + 3 + 1 windows against one call, overall")
    _assert_close(parts.batch_mean, z["a.zero.batch_mean_split"], 1e-5, "batch mean of 3 + 3 + 1")
    assert parts.batches == 3 and not np.allclose(parts.batch_mean, one.batch_mean, rtol=1e-4, atol=0)          # the split does change it
    m.reset()
    repeat = _feed(m, "a", [3, 3, 1])
    _assert_close(repeat.per_horizon, parts.per_horizon, 1e-12, "after reset(), per horizon")
    _assert_close(repeat.overall, parts.overall, 1e-12, "after reset(), overall")
    _assert_close(repeat.batch_mean, parts.batch_mean, 1e-12, "after reset(), batch mean")
    some = m.result(horizons=[2, 11])
    assert some.horizons == (2, 11) and np.array_equal(some.per_horizon, m.result().per_horizon[[2, 11]])
    with pytest.raises(ValueError, match="horizons"):
        m.result(horizons=[12])


def test_layouts_and_refusals():
    z = _fixture()
    pred, real, c = _inputs("b")
    want = _feed(_metrics("b", "zero"), "b", [3])
    m = _metrics("b", "zero")
    m.update(pred.unsqueeze(-1), real[..., c:c + 1])          # [B, H, N, 1] prediction, [B, H, N, 1] slice of the 3-channel label
    got = m.result()
    _assert_close(got.per_horizon, want.per_horizon, 1e-12, "[B, H, N, 1] views")
    m.reset()
    by_node = pred.transpose(1, 2).contiguous()               # stored [B, N, H]
    view = by_node.transpose(1, 2)
    assert view.shape == pred.shape and view.stride() != pred.stride() and not view.is_contiguous()
    m.update(view, real[..., c])
    got = m.result()
    _assert_close(got.per_horizon, want.per_horizon, 1e-12, "prediction as a transposed view of [B, N, H]")
    _assert_close(got.overall, z["b.zero.overall"], 1e-5, "transposed view against the reference")
    # refused before anything is launched; the accumulator is untouched
    before = m.result()
    label = real[..., c]
    for p, r in ((pred[:, :6], label[:, :6]), (pred, label[:2]), (pred[:, :, :299], label), (pred.double(), label), (pred, label.double()),
                 (pred.cpu(), label), (pred, label.cpu()), (pred.reshape(-1), label.reshape(-1)), (pred, real),
                 (pred[:, :, :1].expand(3, 12, 300), label)):
        with pytest.raises(ValueError):
            m.update(p, r)
    after = m.result()
    assert m.batches == 1 and np.array_equal(before.per_horizon, after.per_horizon) and np.array_equal(before.batch_mean, after.batch_mean)


# ---------------------------------------------------------------------------------------------- STEP.evaluate
MEAN, STD = 3.25, 1.75          # scaler of the evaluate tests: the series is standard normal, the metrics are taken on x * STD + MEAN


def _torch_three(p, y, null=0.0):
    """basicts/metrics/{mae,rmse,mape}.py restated in torch f32 (as tests/test_gpu_step.py does for step_masked_metrics)"""
    def mask_of(lab, nv):
        m = (~torch.isclose(lab, torch.tensor(nv).expand_as(lab), atol=5e-5, rtol=0.)).float()
        m = m / m.mean()
        return torch.where(torch.isnan(m), torch.zeros_like(m), m)
    m = mask_of(y, null)
    mae = torch.nan_to_num(torch.abs(p - y) * m, nan=0.0).mean()
    mse = torch.nan_to_num((p - y) ** 2 * m, nan=0.0).mean()
    y0 = torch.where(torch.abs(y) < 1e-4, torch.zeros_like(y), y)
    ape = torch.abs(torch.abs(p - y0) / y0) * mask_of(y0, 0.0)
    mape = torch.where(torch.isnan(ape), torch.zeros_like(ape), ape).mean()
    return [float(mae), float(torch.sqrt(mse)), float(mape)]


def _setup(cache_windows=0):
    from tests.test_gpu_eval_cache import BATCHES, _bytes, _fresh
    model, loader = _fresh("bf16")
    if cache_windows:
        model.eval_cache_bytes = _bytes(cache_windows)
    model.tsformer._events = []
    return model, loader, [t for b in BATCHES for t in b]


def test_evaluate_equals_the_hand_written_loop_and_the_torch_formulas():
    from tests.test_gpu_eval_cache import _reseed
    model, loader, origins = _setup()
    chunks = [origins[0:4], origins[4:8], origins[8:9]]
    _reseed(model)
    by_hand = []
    with torch.no_grad():
        for t0 in chunks:
            hist, ref, _fut = loader.batch(t0)
            by_hand.append(model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=None, epoch=None)[0].clone())
    seeds = (model._seed_ctr, model.tsformer._seed_counter)
    _reseed(model)
    model.train()
    res, preds = model.evaluate(loader, origins, scaler=(MEAN, STD), null_val=0.0, batch_size=4, return_predictions=True)
    assert model.training and model.backend.training          # the previous flag is restored
    model.eval()
    assert (model._seed_ctr, model.tsformer._seed_counter) == seeds and len(model.tsformer._events) == 6
    want = torch.cat(by_hand)[..., 0]
    assert preds.shape == (9, 12, 37) and preds.is_cuda and torch.equal(preds, want)          # bit for bit
    series = loader.data[:, :, 0].cpu()
    label = torch.stack([series[t:t + 12] for t in origins]) * STD + MEAN
    p = want.cpu() * STD + MEAN
    assert res.batches == 3 and res.horizons == tuple(range(12))
    _assert_close(res.per_horizon, [_torch_three(p[:, h], label[:, h]) for h in range(12)], 1e-5, "evaluate per horizon")
    _assert_close(res.overall, _torch_three(p, label), 1e-5, "evaluate overall")
    per_batch = [_torch_three(p[a:b], label[a:b]) for a, b in ((0, 4), (4, 8), (8, 9))]
    _assert_close(res.batch_mean, np.mean(np.array(per_batch, dtype=np.float64), axis=0), 1e-5, "evaluate batch mean")
    # the reference's EVALUATION_HORIZONS; a model in eval() stays in eval()
    _reseed(model)
    some = model.evaluate(loader, origins, scaler={"func": None, "args": {"mean": MEAN, "std": STD}}, batch_size=4, horizons=[2, 5, 11])
    assert not model.training and some.horizons == (2, 5, 11)
    _assert_close(some.per_horizon, res.per_horizon[[2, 5, 11]], 1e-12, "selected horizons")
    with pytest.raises(ValueError, match="host integers"):
        model.evaluate(loader, torch.tensor(origins).cuda())
    with pytest.raises(ValueError, match="origins"):
        model.evaluate(loader)


def test_second_evaluate_with_the_cache_launches_no_encoder():
    from tests.test_gpu_eval_cache import _reseed
    model, loader, origins = _setup(cache_windows=9)
    _reseed(model)
    first, p1 = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4, return_predictions=True)
    assert len(model.tsformer._events) == 3 and model.eval_cache_stats["windows_stored"] == 9
    _reseed(model)
    second, p2 = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4, return_predictions=True)
    assert len(model.tsformer._events) == 3 and model.eval_cache_stats["window_hits"] == 9
    assert torch.equal(p1, p2)          # the bf16-mode evaluation is bit-reproducible at this shape (tests/test_gpu_eval_cache.py)
    _assert_close(second.per_horizon, first.per_horizon, 1e-12, "cached pass, per horizon")
    _assert_close(second.overall, first.overall, 1e-12, "cached pass, overall")
    _assert_close(second.batch_mean, first.batch_mean, 1e-12, "cached pass, batch mean")


def test_evaluate_over_a_device_forecasting_dataset(tmp_path):
    from step_amd.runner import DeviceForecastingDataset
    from tests.test_gpu_eval_cache import _reseed
    model, loader, origins = _setup()
    with open(tmp_path / "data.pkl", "wb") as f:
        pickle.dump({"processed_data": loader.data.cpu().numpy()}, f)
    with open(tmp_path / "index.pkl", "wb") as f:
        pickle.dump({k: [(t - 12, t, t + 12) for t in origins] for k in ("train", "valid", "test")}, f)
    ds = DeviceForecastingDataset(str(tmp_path / "data.pkl"), str(tmp_path / "index.pkl"), "test", loader.long_len)
    _reseed(model)
    want, p_want = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4, return_predictions=True)
    _reseed(model)
    got, p_got = model.evaluate(ds, scaler=(MEAN, STD), batch_size=4, return_predictions=True)
    assert torch.equal(p_got, p_want) and got.batches == want.batches == 3
    assert ds.device_loader(p_got.device) is ds.device_loader(p_got.device)          # the dataset's own loader, built once
    _assert_close(got.per_horizon, want.per_horizon, 1e-12, "dataset, per horizon")
    _assert_close(got.overall, want.overall, 1e-12, "dataset, overall")
    _assert_close(got.batch_mean, want.batch_mean, 1e-12, "dataset, batch mean")
    with pytest.raises(ValueError, match="DeviceWindowLoader"):
        model.evaluate([1, 2, 3], origins)
