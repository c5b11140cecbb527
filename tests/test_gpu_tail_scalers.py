"""The tails under a NaN ``null_val`` and under per-node scalers on the device: ``step_amd.step_loss.train_tail`` (libstep_hip
step_train_tail / step_train_tail_nodes), ``EvalMetrics`` (step_eval_metrics_accumulate / _nodes) and the pre-training tail's kernel entry
behind ``_PretrainTail`` against the reference's own numbers (tests/golden/tail_scaler_cases.npz, recorded by
tools/make_tail_scaler_golden.py; its ``inputs`` builds the tensors from the fixture's arrays), the new entries against their scalar
siblings bit for bit, and ``native_runner`` with an ``ndarray`` scaler and a NaN ``null_val`` against the base class's tail.
Bounds are those of tests/test_gpu_train_tail.py and tests/test_gpu_eval_metrics.py for the scalar tails: loss rel 1e-5, metrics rtol
2e-5 / atol 1e-6, gradients rel_l2 < 1e-5, tables relative 1e-5 (absolute 1e-6 where the reference gives 0); the gradient's non-zero
pattern equals the reference's element for element.  Host side: tests/test_tail_scaler_host.py."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.eval_runner_double import EvalRunnerDouble
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tail_scaler_cases.npz")
NAN = float("nan")
KS = (1, 5, 12)
PAIRS = {"nan_scalar": (NAN, "scalar"), "zero_node": (0.0, "node"), "nan_node": (NAN, "node")}
CASES = [(s, p) for s in ("a", "b", "c", "one") for p in PAIRS] + [("allnan", "nan_node")]


@functools.lru_cache(maxsize=None)
def tool():
    spec = importlib.util.spec_from_file_location("make_tail_scaler_golden", os.path.join(ROOT, "tools", "make_tail_scaler_golden.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@functools.lru_cache(maxsize=None)
def device_case(s, kind):
    """device tensors of one shape under one kind of scaler, uploaded once and left unchanged"""
    z = fixture()
    pred, real = tool().inputs(z, s, kind)
    src = "a" if s == "allnan" else s
    d = {"pred": torch.from_numpy(pred).cuda(), "real": torch.from_numpy(real).cuda(), "nan_at": np.isnan(pred) | np.isnan(real[..., 0])}
    d.update({key: torch.from_numpy(z[f"{src}.{key}"]).cuda() for key in ("theta", "prior")})
    d["coef"] = float(z[f"{src}.coef"])
    d["rescale"] = (float(z["scalar.mean"]), float(z["scalar.std"])) if kind == "scalar" else (z[f"{src}.mean_n"], z[f"{src}.std_n"])
    return d


def run(s, pair, k, label="view", rescale=None, null_val=None, via_loss=False):
    """-> (loss, metrics, dpred [B, 12, N], dtheta) of shape s under the pair on the device"""
    from step_amd.step_loss import step_loss_native, train_tail
    nv, kind = PAIRS[pair]
    d = device_case(s, kind)
    pred = d["pred"][..., None].clone().requires_grad_(True)
    theta = d["theta"].clone().requires_grad_(True)
    real = d["real"][..., :1]                                  # channel 0 of [B, 12, N, C], in place
    if label == "contiguous":
        real = real.contiguous()
    kw = dict(null_val=nv if null_val is None else null_val, rescale=d["rescale"] if rescale is None else rescale)
    if via_loss:
        loss, metrics = step_loss_native(pred, real, theta, d["prior"], d["coef"], **kw), None
    else:
        loss, metrics = train_tail(pred, real, theta, d["prior"], d["coef"], horizons=k, **kw)
        assert not metrics.requires_grad and metrics.dtype == torch.float32 and metrics.shape == (3,)
    dp, dt = torch.autograd.grad(loss, [pred, theta])
    return loss.detach(), metrics, dp[..., 0], dt


@functools.lru_cache(maxsize=None)
def result(s, pair, k):
    return run(s, pair, k)


def same_bits(xs, ys):
    return all(torch.equal(x, y) for x, y in zip(xs, ys) if x is not None and y is not None)


# ---------------------------------------------------------------------------------------------- the training tail against the reference
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("s,pair", CASES)
def test_train_tail_against_the_reference(s, pair, k):
    z = fixture()
    loss, metrics, dp, dt = result(s, pair, k)
    want_loss, want_metrics = float(z[f"{s}.{pair}.{k}.loss"]), z[f"{s}.{pair}.{k}.metrics"]
    print(s, pair, k, "loss", float(loss), want_loss, "metrics", metrics.tolist(), want_metrics.tolist())
    assert float(loss) == pytest.approx(want_loss, rel=1e-5)
    assert torch.allclose(metrics.cpu(), torch.from_numpy(want_metrics), rtol=2e-5, atol=1e-6)
    src = "a" if s == "allnan" else s
    assert rel_l2(dt.cpu(), torch.from_numpy(z[f"{src}.dtheta"])) < 1e-5
    dp = dp.cpu()
    nan_at = torch.from_numpy(device_case(s, PAIRS[pair][1])["nan_at"])
    want = torch.from_numpy(z[f"{s}.{pair}.{k}.dpred"]).clone()
    assert torch.isfinite(dp).all() and (dp[:, k:] == 0).all()          # excluded horizons: written, and exactly zero
    assert (dp[nan_at] == 0).all() and bool(nan_at.any())
    want[nan_at] = 0.0          # (the reference's gradient of a NaN term is NaN; here it is defined as 0)
    assert torch.equal(dp != 0, want != 0)                               # the bit-exact mask: the same labels masked, element for element
    if float(want.abs().max()) == 0.0:                                   # nothing counts: the graph term alone
        assert (s, k) == ("allnan", 1) and float(dp.abs().max()) == 0.0 and metrics.tolist() == [0.0, 0.0, 0.0] and float(loss) > 0
    else:
        print(s, pair, k, "rel_l2 dpred", rel_l2(dp, want))
        assert rel_l2(dp, want) < 1e-5


# ---------------------------------------------------------------------------------------------- the evaluation accumulator
def _assert_close(got, want, rel, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.where(want == 0.0, 1e-6, rel * np.abs(want))
    err = np.abs(got - want)
    print(f"{what}: largest |difference| / bound = {float(np.max(err / bound)):.3e}")
    assert got.shape == want.shape and np.all(err <= bound), (what, got, want)


def feed(s, pair, split, rescale=None):
    from step_amd import EvalMetrics
    nv, kind = PAIRS[pair]
    d = device_case(s, kind)
    mean, std = d["rescale"] if rescale is None else rescale
    m = EvalMetrics(horizons=12, null_val=nv, rescale=(std, mean))
    at = 0
    for n in split:
        m.update(d["pred"][at:at + n], d["real"][at:at + n, :, :, 0])
        at += n
    assert at == d["pred"].shape[0]
    return m.result()


@pytest.mark.parametrize("s,pair", CASES)
def test_eval_metrics_against_the_reference(s, pair):
    z = fixture()
    src = "a" if s == "allnan" else s
    B = z[f"{src}.raw"].shape[0]
    one = feed(s, pair, [B])
    _assert_close(one.per_horizon, z[f"{s}.{pair}.per_horizon"], 1e-5, f"{s}/{pair} per horizon")
    _assert_close(one.overall, z[f"{s}.{pair}.overall"], 1e-5, f"{s}/{pair} overall")
    split = tool().SPLITS[s]
    parts = feed(s, pair, split)
    assert parts.batches == len(split)
    _assert_close(parts.per_horizon, z[f"{s}.{pair}.per_horizon"], 1e-5, f"{s}/{pair} per horizon, split {split}")
    _assert_close(parts.batch_mean, z[f"{s}.{pair}.batch_mean_split"], 1e-5, f"{s}/{pair} batch mean, split {split}")
    if s == "allnan":
        assert (one.per_horizon[0] == 0.0).all()          # the all-NaN horizon: a count of 0 gives exactly 0


# ---------------------------------------------------------------------------------------------- the pre-training tail
@functools.lru_cache(maxsize=None)
def pretrain_case(c):
    z = fixture()
    return {key: torch.from_numpy(z[f"{c}.{key}"]).cuda() for key in ("r", "series", "mk")}


def run_pretrain(c, null_val=NAN):
    from step_amd.step_arch.tsformer import _PretrainTail
    z, d = fixture(), pretrain_case(c)
    r = d["r"].clone().requires_grad_(True)
    loss, metrics = _PretrainTail.apply(r, d["series"], d["mk"], null_val, float(z["scalar.std"]), float(z["scalar.mean"]), True)
    dr, = torch.autograd.grad(loss, [r])
    return loss.detach(), metrics, dr


@pytest.mark.parametrize("c", ("p18", "p5"))
def test_pretrain_tail_under_a_nan_null_val_against_the_reference(c):
    z = fixture()
    loss, metrics, dr = run_pretrain(c)
    print(c, "loss", float(loss), float(z[f"{c}.loss"]), "metrics", metrics.tolist(), z[f"{c}.metrics"].tolist())
    assert float(loss) == pytest.approx(float(z[f"{c}.loss"]), rel=1e-5)
    assert torch.allclose(metrics.cpu(), torch.from_numpy(z[f"{c}.metrics"]), rtol=2e-5, atol=1e-6)
    S, P, _ = z[f"{c}.r"].shape
    Pu, mk = int(z[f"{c}.Pu"]), z[f"{c}.mk"].astype(np.int64)
    nan_at = np.isnan(z[f"{c}.r"])
    nan_at[:, Pu:, :] |= np.isnan(z[f"{c}.series"].reshape(S, P, 12)[:, mk, :])
    nan_at = torch.from_numpy(nan_at)
    dr, want = dr.cpu(), torch.from_numpy(z[f"{c}.dr"]).clone()
    assert torch.isfinite(dr).all() and (dr[:, :Pu] == 0).all() and (dr[nan_at] == 0).all() and int(nan_at.sum()) == 6
    want[nan_at] = 0.0
    assert torch.equal(dr != 0, want != 0)
    print(c, "rel_l2 dr", rel_l2(dr, want))
    assert rel_l2(dr, want) < 1e-5
    # zeros are labels like any other under a NaN null_val: the finite rule on the same tensors masks them and gives another loss
    assert float(run_pretrain(c, null_val=0.0)[0]) != float(loss)
    # TSFormer.pretrain_tail hands None over as NaN, and still refuses a float NaN (tests/test_pretrain_tail_host.py)


# ---------------------------------------------------------------------------------------------- bit-identical siblings
@pytest.mark.parametrize("s,pair,k", [("b", "nan_node", 5), ("c", "zero_node", 12), ("c", "nan_scalar", 1), ("one", "nan_node", 12)])
def test_label_view_and_its_contiguous_copy_give_identical_bits(s, pair, k):
    assert same_bits(result(s, pair, k), run(s, pair, k, label="contiguous"))


@pytest.mark.parametrize("null_val", (0.0, NAN), ids=("zero", "nan"))
@pytest.mark.parametrize("s,k", [("a", 5), ("c", 12), ("c", 1), ("one", 1)])
def test_equal_node_entries_give_the_bits_of_the_scalar_entry(s, k, null_val):
    """a per-node scaler whose N entries are all equal, through step_train_tail_nodes / step_eval_metrics_accumulate_nodes, against the
    scalar entries on the same inputs"""
    z = fixture()
    N = z[f"{s}.raw"].shape[2]
    mean, std = float(z["scalar.mean"]), float(z["scalar.std"])
    arrays = (np.full((1, N, 1), mean), np.full((1, N, 1), std))
    scalar = run(s, "nan_scalar", k, null_val=null_val)
    for rescale in (arrays, (mean, arrays[1]), (torch.from_numpy(arrays[0]).reshape(N), std)):          # a scalar next to an array is broadcast
        assert same_bits(scalar, run(s, "nan_scalar", k, null_val=null_val, rescale=rescale))
    a, b = feed(s, "nan_scalar", tool().SPLITS[s]), feed(s, "nan_scalar", tool().SPLITS[s], rescale=arrays)          # (feeds a NaN null_val)
    if null_val != null_val:
        # f64 sums of identical f32 terms in launches of one shape; only the order of the workgroups' atomic adds may differ
        # (relative 1e-12, the bound of tests/test_gpu_eval_metrics.py for two ways of accumulating the same elements)
        for x, y, what in ((a.per_horizon, b.per_horizon, "per horizon"), (a.overall, b.overall, "overall"), (a.batch_mean, b.batch_mean, "batch mean")):
            _assert_close(y, x, 1e-12, f"{s} equal node entries against the scalar entry, {what}")


def raw_tail(entry, d, k, scaler, null_val):
    """one call of a libstep_hip training-tail entry on a work buffer of its own -> (loss, metrics, dpred, dtheta)"""
    from step_amd import _lib
    p, r = d["pred"], d["real"]
    B, H, N = p.shape
    C = r.shape[3]
    work = torch.zeros(_lib.lib().step_train_tail_work_doubles(), dtype=torch.float64, device="cuda")
    loss, metrics = torch.empty((), device="cuda"), torch.empty(3, device="cuda")
    dp, dt = torch.empty(B, H, N, device="cuda"), torch.empty_like(d["theta"])
    _lib.call(entry, _lib.ptr(p), H * N, N, 1, ctypes.c_void_p(r.data_ptr()), H * N * C, N * C, C, B, H, N, k, *scaler, null_val,
              _lib.ptr(d["theta"]), _lib.ptr(d["prior"]), d["theta"].numel(), d["coef"], _lib.ptr(work), _lib.ptr(loss), _lib.ptr(metrics),
              _lib.ptr(dp), _lib.ptr(dt), _lib.stream())
    return loss, metrics, dp, dt


@pytest.mark.parametrize("c", ("a", "b", "c", "d", "e0"))
def test_a_finite_null_val_gives_todays_bits_on_the_stored_scalar_cases(c):
    """tests/golden/train_tail_cases.npz through the changed tails: ``train_tail`` and the per-node entry with equal entries against the
    scalar entry called directly on the same inputs; the values themselves are held to the reference by tests/test_gpu_train_tail.py"""
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", "train_tail_cases.npz")))
    from step_amd.step_loss import train_tail
    d = {key: torch.from_numpy(z[f"{c}.{key}"]).cuda() for key in ("pred", "real", "theta", "prior")}
    d["coef"] = float(z[f"{c}.coef"])
    scale, shift = float(z[f"{c}.scale"]), float(z[f"{c}.shift"])
    N = d["pred"].shape[2]
    for k in (5, 12):
        direct = raw_tail("step_train_tail", d, k, (scale, shift), 0.0)
        pred, theta = d["pred"][..., None].clone().requires_grad_(True), d["theta"].clone().requires_grad_(True)
        loss, metrics = train_tail(pred, d["real"][..., :1], theta, d["prior"], d["coef"], null_val=0.0, rescale=(shift, scale), horizons=k)
        dp, dt = torch.autograd.grad(loss, [pred, theta])
        assert same_bits(direct, (loss.detach(), metrics, dp[..., 0], dt))
        from step_amd import _lib
        sn, hn = torch.full((N,), scale, device="cuda"), torch.full((N,), shift, device="cuda")
        assert same_bits(direct, raw_tail("step_train_tail_nodes", d, k, (_lib.ptr(sn), _lib.ptr(hn)), 0.0))


@pytest.mark.parametrize("s,pair", [("b", "nan_scalar"), ("c", "nan_node"), ("a", "zero_node")])
def test_step_loss_native_goes_through_train_tail(s, pair):
    via = run(s, pair, None, via_loss=True)
    full = result(s, pair, 12)
    assert torch.equal(via[0], full[0]) and torch.equal(via[2], full[2]) and torch.equal(via[3], full[3])


def test_masked_mae_native_under_a_nan_null_val():
    from step_amd.step_loss import masked_mae, masked_mae_native
    d = device_case("b", "scalar")
    pred = d["pred"].transpose(1, 2).clone().requires_grad_(True)          # [B, N, 12]: any shape, any contiguous layout
    label = d["real"][..., 0].transpose(1, 2).contiguous()
    loss = masked_mae_native(pred, label, null_val=NAN, rescale=d["rescale"])
    g, = torch.autograd.grad(loss, [pred])
    p2 = pred.detach().clone().requires_grad_(True)
    mean, std = d["rescale"]
    want = masked_mae(p2 * std + mean, label * std + mean, NAN)
    g2, = torch.autograd.grad(want, [p2])
    assert float(loss.detach()) == pytest.approx(float(want.detach()), rel=1e-5) and g.shape == pred.shape
    g2 = torch.nan_to_num(g2, nan=0.0)
    assert rel_l2(g.cpu(), g2.cpu()) < 1e-5


def test_wrong_lengths_and_null_values_raise():
    from step_amd import EvalMetrics
    from step_amd.step_loss import train_tail
    d = device_case("a", "node")
    args = (d["pred"][..., None], d["real"][..., :1], d["theta"], d["prior"], 1.0)
    N = d["pred"].shape[2]
    for bad in (np.ones(N + 1), np.ones((1, N - 1, 1)), np.ones((N, N)), torch.ones(2 * N)):
        with pytest.raises(ValueError, match="non-unit dimensions"):
            train_tail(*args, rescale=(bad, np.ones(N)))
        with pytest.raises(ValueError, match="non-unit dimensions"):
            EvalMetrics(12, rescale=(np.ones(N), bad)).update(d["pred"], d["real"][..., 0])
    for nv in (float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            train_tail(*args, null_val=nv)
    with pytest.raises(ValueError, match="finite"):
        train_tail(*args, rescale=(np.full(N, NAN), np.ones(N)))


# ---------------------------------------------------------------------------------------------- the runner
def _mask(labels, null_val):
    """basicts/metrics/mae.py:17-21"""
    if np.isnan(null_val):
        m = ~torch.isnan(labels)
    else:
        m = ~torch.isclose(labels, torch.tensor(null_val).expand_as(labels).to(labels.device), atol=5e-5, rtol=0.)
    m = m.float()
    m = m / torch.mean(m)
    return torch.where(torch.isnan(m), torch.zeros_like(m), m)


def masked_mae(preds, labels, null_val=np.nan):
    loss = torch.abs(preds - labels) * _mask(labels, null_val)
    return torch.mean(torch.where(torch.isnan(loss), torch.zeros_like(loss), loss))


def masked_rmse(preds, labels, null_val=np.nan):
    loss = (preds - labels) ** 2 * _mask(labels, null_val)
    return torch.sqrt(torch.mean(torch.where(torch.isnan(loss), torch.zeros_like(loss), loss)))


def masked_mape(preds, labels, null_val=np.nan):
    labels = torch.where(torch.abs(labels) < 1e-4, torch.zeros_like(labels), labels)
    loss = torch.abs(torch.abs(preds - labels) / labels) * _mask(labels, 0.0)
    return torch.mean(torch.where(torch.isnan(loss), torch.zeros_like(loss), loss))


masked_mae.__module__, masked_rmse.__module__, masked_mape.__module__ = "basicts.metrics.mae", "basicts.metrics.rmse", "basicts.metrics.mape"


def re_standard_transform(data, mean, std):
    """basicts/data/transform.py:59-65"""
    if isinstance(mean, np.ndarray):
        mean = torch.from_numpy(mean).type_as(data).to(data.device).unsqueeze(0)
        std = torch.from_numpy(std).type_as(data).to(data.device).unsqueeze(0)
    return data * std + mean


class ArrayScalerDouble(EvalRunnerDouble):
    """the runner double with the reference's NaN-aware metrics and its ``re_standard_transform`` for ``ndarray`` arguments in both
    base tails (base_tsf_runner.py:237-255, :257-273)"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.metrics = {"MAE": masked_mae, "RMSE": masked_rmse, "MAPE": masked_mape}
        self.null_val = cfg["null_val"]

    def train_iters(self, epoch, iter_index, data):
        self.base_calls += 1
        iter_num = (epoch - 1) * self.iter_per_epoch + iter_index
        forward_return = list(self.forward(data=data, epoch=epoch, iter_num=iter_num, train=True))
        forward_return[0] = re_standard_transform(forward_return[0], **self.scaler["args"])
        forward_return[1] = re_standard_transform(forward_return[1], **self.scaler["args"])
        if self.cl_param:
            cl_length = self.curriculum_learning(epoch=epoch)
            forward_return[0] = forward_return[0][:, :cl_length, :, :]
            forward_return[1] = forward_return[1][:, :cl_length, :, :]
        loss = self.metric_forward(self.loss, forward_return)
        for metric_name, metric_func in self.metrics.items():
            metric_item = self.metric_forward(metric_func, forward_return[:2])
            self.update_epoch_meter("train_" + metric_name, metric_item.item())
        return loss

    def val_iters(self, iter_index, data):
        self.val_base_calls += 1
        forward_return = self.forward(data=data, epoch=None, iter_num=None, train=False)
        prediction_rescaled = re_standard_transform(forward_return[0], **self.scaler["args"])
        real_value_rescaled = re_standard_transform(forward_return[1], **self.scaler["args"])
        for metric_name, metric_func in self.metrics.items():
            metric_item = self.metric_forward(metric_func, [prediction_rescaled, real_value_rescaled])
            self.update_epoch_meter("val_" + metric_name, metric_item.item())


CL = {"WARM_EPOCHS": 0, "CL_EPOCHS": 1, "PREDICTION_LENGTH": 12}
NAMES = ("MAE", "RMSE", "MAPE")


def node_arrays(shape="per_node"):
    from tests.test_gpu_train_tail import tiny
    g, model, batch = tiny()
    mean, std = [float(x) for x in g["meta.scaler"]]
    N = batch[0].shape[2]
    mean_n, std_n = mean + np.linspace(-0.2, 0.2, N) * std, std * np.linspace(0.8, 1.25, N)
    return (mean_n.reshape(1, N, 1), std_n.reshape(1, N, 1)) if shape == "per_node" else (mean_n, std_n)


def runner(native, scaler, cl=None):
    from step_amd.runner import native_runner
    from step_amd.step_loss import step_loss
    from tests.test_gpu_train_tail import tiny
    _g, model, batch = tiny()
    r = native_runner(ArrayScalerDouble, native_tail=native, native_eval=native)(
        {"model": model, "loss": step_loss, "scaler": scaler, "cl": cl, "null_val": NAN})
    return r, model, batch


def train_once(native, scaler, cl, epoch):
    r, model, batch = runner(native, scaler, cl)
    model.train()
    model.zero_grad(set_to_none=True)
    loss = r.train_iters(epoch, 0, batch)
    loss.backward()
    grad = model._flat_grad.clone()
    r.flush_meters()
    return float(loss), {k: r.meters["train_" + k].avg for k in NAMES}, grad, r


@pytest.mark.parametrize("cl,epoch", [(CL, 5), (None, 1)])
def test_runner_takes_the_native_tail_under_an_array_scaler_and_a_nan_null_val(cl, epoch):
    scaler = node_arrays()
    l0, m0, g0, r0 = train_once(False, scaler, cl, epoch)
    l1, m1, g1, r1 = train_once(True, scaler, cl, epoch)
    rel = float((g1 - g0).norm() / g0.norm())
    print("cl", cl is not None, "loss", l0, l1, "meters", m0, m1, "relative L2 of the flat gradients", rel)
    assert r0.base_calls == 1 and r1.base_calls == 0 and r1._tail_scaler() is not None
    assert l1 == pytest.approx(l0, rel=1e-5)
    for k in m0:
        assert m1[k] == pytest.approx(m0[k], rel=2e-5)
    assert float(g0.norm()) > 0 and rel <= 1e-3
    # the per-node scaler matters on this batch: the scalar one gives another loss
    from tests.helpers import load_golden
    mean, std = [float(x) for x in load_golden("step_tiny")["meta.scaler"]]
    assert abs(train_once(True, (mean, std), cl, epoch)[0] - l1) > 1e-3 * l1


def validate_once(native, scaler):
    r, model, batch = runner(native, scaler)
    r.val_data_loader = [batch, batch]
    r.reset_epoch_meters()
    r.validate(train_epoch=1)
    model.train()
    return {k: r.meters["val_" + k].avg for k in NAMES}, r


def test_runner_takes_the_native_validation_under_an_array_scaler_and_a_nan_null_val():
    scaler = node_arrays()
    m1, r1 = validate_once(True, scaler)
    assert r1.val_base_calls == 0 and r1.eval_readbacks == 1 and [n for _name, _v, n in r1.meter_log] == [2, 2, 2]
    # the base class's formulas on the pass's own predictions (the graph learner samples in eval mode too)
    _fut = r1.to_running_device(r1.val_data_loader[0][0])
    real = re_standard_transform(_fut[..., :1], *scaler)
    rows = [[float(f(re_standard_transform(p, *scaler), real, null_val=NAN)) for f in (masked_mae, masked_rmse, masked_mape)]
            for p in r1.predictions]
    want = dict(zip(NAMES, np.mean(np.array(rows, dtype=np.float64), axis=0)))
    print("val meters", m1, "expected", want)
    for k in NAMES:
        assert m1[k] == pytest.approx(want[k], rel=2e-5)
    m0, r0 = validate_once(False, scaler)
    assert r0.val_base_calls == 2


def test_runner_keeps_the_base_path_for_a_flat_array_scaler():
    """shape (N,): the reference broadcasts it against the LAST dimension -- not a per-node scaler, the base class's business"""
    flat = node_arrays("flat")
    r, model, batch = runner(True, flat)
    assert r._scaler_mean_std() is None and r._tail_scaler() is None and r._eval_scaler() is None
    model.train()
    model.zero_grad(set_to_none=True)
    loss = r.train_iters(1, 0, batch)
    r.flush_meters()
    assert r.base_calls == 1 and torch.isfinite(loss) and r.meters["train_MAE"].n == 1
    r.val_data_loader = [batch]
    r.reset_epoch_meters()
    r.validate(train_epoch=1)
    model.train()
    assert r.val_base_calls == 1 and r.eval_readbacks == 0 and r.meters["val_MAE"].n == 1


def test_runner_checks_the_scaler_length_against_the_forward_before_any_launch(monkeypatch):
    import step_amd.step_loss as SL
    mean_n, std_n = node_arrays()
    twice = (np.concatenate([mean_n, mean_n], axis=1), np.concatenate([std_n, std_n], axis=1))          # [1, 2 N, 1]
    r, model, batch = runner(True, twice)
    assert r._tail_scaler() is not None          # a per-node scaler as far as anything known before the forward goes
    monkeypatch.setattr(SL, "train_tail", lambda *a, **k: pytest.fail("train_tail was called"))
    model.train()
    model.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match="must match"):          # the torch tail of the fall-back: 2 N against N does not broadcast, as in the reference
        r.train_iters(1, 0, batch)
    model.zero_grad(set_to_none=True)
