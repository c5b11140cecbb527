"""Host side of the tails under a NaN ``null_val`` and per-node scalers (tests/test_gpu_tail_scalers.py has the device side): the
fixture tests/golden/tail_scaler_cases.npz says what its recording tool promises (every slice counts at least half of its labels, the
results are finite, the reference's gradient is exactly zero at masked labels and excluded horizons), the tool reproduces it where the
reference is at hand, and ``native_runner``'s conditions accept and reject the scalers and null values they should -- none of which
needs a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle.reference_loader import reference_root
from tests.test_abi_and_host import _DummyBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tail_scaler_cases.npz")
NAN = float("nan")


def tool():
    spec = importlib.util.spec_from_file_location("make_tail_scaler_golden", os.path.join(ROOT, "tools", "make_tail_scaler_golden.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


def rescaled(t, z, name, kind):
    """-> (p, y, masked) f32 [B, 12, N]: x * std + mean of both tensors as torch rounds it, and the NaN positions of either"""
    pred, real = t.inputs(z, name, kind)
    src = "a" if name == "allnan" else name
    N = pred.shape[2]
    if kind == "scalar":
        mean, std = torch.tensor(float(z["scalar.mean"])), torch.tensor(float(z["scalar.std"]))
    else:
        mean, std = (torch.from_numpy(z[f"{src}.{key}"].reshape(N)).float() for key in ("mean_n", "std_n"))
    p, y = torch.from_numpy(pred) * std + mean, torch.from_numpy(real[..., 0]) * std + mean
    return p, y, torch.isnan(p) | torch.isnan(y)


def test_fixture_is_consistent_with_itself():
    t, z = tool(), dict(np.load(FIXTURE))
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "train_tail_cases.npz"))
    assert list(z["shapes"]) == list(t.SHAPES) + ["allnan"] and tuple(z["ks"]) == t.KS == (1, 5, 12) and list(z["pairs"]) == list(t.PAIRS)
    for name, (B, N, C) in t.SHAPES.items():
        assert z[f"{name}.raw"].shape == (B, 12, N) and int(z[f"{name}.C"]) == C and int(z[f"{name}.split"].sum()) == B
        mean, std = z[f"{name}.mean_n"], z[f"{name}.std_n"]
        assert mean.shape == std.shape == (1, N, 1) and mean.dtype == std.dtype == np.float64
        assert (150 <= mean).all() and (mean <= 250).all() and (20 <= std).all() and (std <= 80).all()
        if N > 1:
            assert len(np.unique(mean)) == N and len(np.unique(std)) == N          # no two nodes alike: a swapped index shows
        raw = z[f"{name}.raw"]
        if raw.size > 24:
            assert 0.1 < float((raw == 0).mean()) < 0.3 and int(((raw > 0) & (raw < 1e-3)).sum()) >= 20 and len(z[f"{name}.nan_labels"]) == 5
    for name in z["shapes"]:
        for pair in t.pairs_of(name):
            null_val, kind = t.PAIRS[pair]
            p, y, nan_at = rescaled(t, z, name, kind)
            kept = t.counted(y, null_val)
            assert int(torch.isnan(p).sum()) == 1
            assert name == "allnan" or bool(kept[torch.isnan(p)].all())          # the NaN prediction sits on a counted label
            for k in t.KS:
                share = float(kept[:, :k].float().mean())
                loss, metrics, dpred = (z[f"{name}.{pair}.{k}.{key}"] for key in ("loss", "metrics", "dpred"))
                assert np.isfinite(loss) and np.isfinite(metrics).all() and loss > 0
                assert (np.isfinite(dpred) | nan_at.numpy()).all()
                assert (dpred[:, k:][~nan_at[:, k:].numpy()] == 0).all()                       # excluded horizons
                assert (dpred[:, :k][(~kept[:, :k] & ~nan_at[:, :k]).numpy()] == 0).all()      # masked labels
                if (name, k) == ("allnan", 1):
                    assert share == 0.0 and (metrics == 0).all() and (dpred[~nan_at.numpy()] == 0).all()
                else:
                    assert share >= 0.5 and (metrics > 0).all()
                    inc = (kept & ~nan_at)[:, :k].numpy()
                    assert (dpred[:, :k][inc] != 0).all()          # (no prediction equals its label)
            table = z[f"{name}.{pair}.per_horizon"]
            assert table.shape == (12, 3) and np.isfinite(table).all() and np.isfinite(z[f"{name}.{pair}.overall"]).all()
            assert z[f"{name}.{pair}.batch_mean_split"].shape == (3,)
    # the pairs differ where they should: zeros are masked under null_val = 0.0 and counted under NaN
    assert z["c.zero_node.12.loss"] != z["c.nan_node.12.loss"]
    assert z["allnan.nan_node.1.loss"] < z["a.nan_node.1.loss"]
    for name in z["pretrain_cases"]:
        S, P, _ = z[f"{name}.r"].shape
        Pu, mk = int(z[f"{name}.Pu"]), z[f"{name}.mk"]
        assert (S, P, P - Pu) in ((18, 16, 12), (5, 8, 6)) and len(mk) == P - Pu and S == int(z[f"{name}.B"]) * int(z[f"{name}.N"])
        lab = z[f"{name}.series"].reshape(S, P, 12)[:, mk, :]
        assert int(np.isnan(lab).sum()) == 5 and int(np.isnan(z[f"{name}.r"]).sum()) == 1 and float((~np.isnan(lab)).mean()) >= 0.5
        dr = z[f"{name}.dr"]
        nan_at = np.isnan(z[f"{name}.r"])
        nan_at[:, Pu:, :] |= np.isnan(lab)
        assert np.isfinite(z[f"{name}.loss"]) and (z[f"{name}.metrics"] > 0).all() and (np.isfinite(dr) | nan_at).all()
        assert (dr[:, :Pu][~nan_at[:, :Pu]] == 0).all() and (dr[:, Pu:][~nan_at[:, Pu:]] != 0).all()


@pytest.mark.skipif(reference_root() is None, reason="needs the reference sources")
def test_recording_tool_reproduces_the_stored_fixture():
    got, z = tool().compute(), np.load(FIXTURE)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        a, b = np.asarray(got[key]), z[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if key.split(".")[-1] in ("loss", "metrics", "dpred", "dtheta", "dr", "per_horizon", "overall", "batch_mean_split"):
            # results: f32 sums on another CPU may be ordered differently
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-12, err_msg=key)
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


# ---------------------------------------------------------------------------------------------- native_runner's conditions
def masked_mae(preds, labels, null_val=NAN):
    return (preds - labels).abs().mean()


def masked_rmse(preds, labels, null_val=NAN):
    return (preds - labels).pow(2).mean().sqrt()


masked_mae.__module__, masked_rmse.__module__ = "basicts.metrics.mae", "basicts.metrics.rmse"


def step_loss(*args, **kwargs):
    raise AssertionError("not called")


def runner_with(mean, std, null_val=0.0):
    from step_amd.runner import native_runner
    r = native_runner(_DummyBase, native_tail=True, native_eval=True)({})
    r.scaler = {"func": "re_standard_transform", "args": {"mean": mean, "std": std}}
    r.metrics = {"MAE": masked_mae, "RMSE": masked_rmse}
    r.loss = step_loss
    r.null_val = null_val
    return r


def test_scaler_mean_std_accepts_scalars_and_per_node_arrays_only():
    N = 7
    mean, std = np.linspace(150.0, 250.0, N).reshape(1, N, 1), np.linspace(20.0, 80.0, N).reshape(1, N, 1)
    assert runner_with(207.5, 38.25)._scaler_mean_std() == (207.5, 38.25)
    assert runner_with(np.float64(207.5), np.float32(38.25))._scaler_mean_std() == (207.5, 38.25)          # numpy scalars are real numbers
    for m, s in ((mean, std), (mean.reshape(N, 1), std.reshape(N, 1)), (mean.astype(np.float32), std.astype(np.float32))):
        got = runner_with(m, s)._scaler_mean_std()
        assert got is not None and got[0] is m and got[1] is s          # the arrays themselves
    rejected = [(mean.reshape(N), std.reshape(N)),                        # (N,): the reference broadcasts it against the LAST dimension
                (mean.reshape(1, 1, N), std.reshape(1, 1, N)), (mean.reshape(N, 1, 1), std.reshape(N, 1, 1)),
                (mean.reshape(1, 1, N, 1), std.reshape(1, 1, N, 1)), (mean, std[:, :3]), (mean, 38.25), (207.5, std),
                (torch.from_numpy(mean), torch.from_numpy(std)), (torch.tensor(207.5), torch.tensor(38.25)),
                (mean.astype(np.int64), std.astype(np.int64)), (np.full((1, N, 1), NAN), std), (True, 38.25), (None, None), ("1", "2")]
    for m, s in rejected:
        assert runner_with(m, s)._scaler_mean_std() is None, (type(m), getattr(m, "shape", None))
    r = runner_with(mean, std)
    r.scaler["func"] = "re_min_max_transform"
    assert r._scaler_mean_std() is None
    r.scaler = (mean, std)
    assert r._scaler_mean_std() is None
    # N against the forward's prediction
    R = type(runner_with(mean, std))
    assert R._scaler_fits((mean, std), torch.zeros(2, 12, N, 1)) and not R._scaler_fits((mean, std), torch.zeros(2, 12, N + 1, 1))
    assert not R._scaler_fits((mean, std), torch.zeros(2, 12, N)) and R._scaler_fits((207.5, 38.25), torch.zeros(2, 12, N + 1, 1))
    x = torch.arange(2.0 * 12 * N).view(2, 12, N, 1)
    assert torch.equal(R._rescaled(x, mean, std), x * torch.from_numpy(std).float()[None] + torch.from_numpy(mean).float()[None])
    assert torch.equal(R._rescaled(x, 207.5, 38.25), x * 38.25 + 207.5)


def test_scalar_rescale_accepts_nan_and_rejects_infinity_and_bool():
    names = ("step_loss", "step_loss_native")
    N = 4
    arrays = (np.full((1, N, 1), 200.0), np.full((1, N, 1), 30.0))
    for scaler in ((207.5, 38.25), arrays):
        assert runner_with(*scaler, null_val=0.0)._scalar_rescale(names) is not None
        got = runner_with(*scaler, null_val=NAN)._scalar_rescale(names)
        assert got is not None and got[0] is scaler[0] or got == (207.5, 38.25)
        assert runner_with(*scaler, null_val=np.float32(NAN))._scalar_rescale(names) is not None
        for bad in (float("inf"), float("-inf"), True, False, None, "nan", torch.tensor(0.0)):
            assert runner_with(*scaler, null_val=bad)._scalar_rescale(names) is None, bad
    assert runner_with(207.5, 38.25, null_val=NAN)._scalar_rescale(("masked_mae",)) is None          # another loss
    r = runner_with(207.5, 38.25, null_val=NAN)
    r.metrics["MSE"] = lambda a, b, null_val=0.0: ((a - b) ** 2).mean()
    assert r._scalar_rescale(names) is None          # a metric that is not one of basicts' three
    # no STEP module on a GPU: the switches stay off whatever the scaler
    assert runner_with(*arrays, null_val=NAN)._tail_scaler() is None and runner_with(*arrays, null_val=NAN)._eval_scaler() is None


def test_val_accumulator_key_tells_array_scalers_apart(monkeypatch):
    import step_amd.evaluate as E
    made = []

    class FakeMetrics:
        batches = 0

        def __init__(self, horizons, null_val, rescale=None, device=None):
            made.append(rescale)

    monkeypatch.setattr(E, "EvalMetrics", FakeMetrics)
    N = 4
    m1, s1 = np.full((1, N, 1), 200.0), np.full((1, N, 1), 30.0)
    m2, s2 = m1.copy(), s1.copy()
    r = runner_with(m1, s1, null_val=NAN)
    a = r._val_accumulator(12, m1, s1, "cuda:0")
    assert r._val_accumulator(12, m1, s1, "cuda:0") is a and len(made) == 1          # the same arrays: the same accumulator (NaN null_val too)
    b = r._val_accumulator(12, m2, s2, "cuda:0")
    assert b is not a and len(made) == 2 and made[1][0] is s2 and made[1][1] is m2          # other arrays (equal or not): a new one
    c = r._val_accumulator(12, 200.0, 30.0, "cuda:0")
    assert c is not b and r._val_accumulator(12, 200.0, 30.0, "cuda:0") is c and len(made) == 3


def test_node_scaler_shapes_are_checked_on_the_host():
    """the length check of ``step_loss.node_scaler`` comes before anything touches a device"""
    from step_amd.step_loss import _is_scalar, node_scaler
    assert node_scaler(207.5, 38.25, 5, torch.device("cpu"), "t") is None and node_scaler(np.float64(1.0), torch.tensor(2.0), 5, None, "t") is None
    assert _is_scalar(3) and _is_scalar(np.float32(3)) and _is_scalar(np.zeros(())) and not _is_scalar(np.zeros(1)) and not _is_scalar(torch.zeros(3))
    for bad in (np.zeros(4), np.zeros((1, 6, 1)), np.zeros((5, 5)), np.zeros((1, 1)), torch.zeros(4)):
        with pytest.raises(ValueError, match="non-unit dimensions"):
            node_scaler(bad, 38.25, 5, torch.device("cpu"), "t")
        with pytest.raises(ValueError, match="non-unit dimensions"):
            node_scaler(207.5, bad, 5, torch.device("cpu"), "t")


def test_scale_shift_hands_array_scalers_through():
    from step_amd.evaluate import _scale_shift
    mean, std = np.full((1, 5, 1), 200.0), np.full((1, 5, 1), 30.0)
    for scaler in ((mean, std), {"mean": mean, "std": std}, {"func": "re_standard_transform", "args": {"mean": mean, "std": std}}):
        got = _scale_shift(scaler)
        assert got[0] is std and got[1] is mean          # (scale, shift) = (std, mean); EvalMetrics checks them against the data's N
    got = _scale_shift((200.0, std))
    assert got[0] is std and got[1] == 200.0          # a scalar next to an array is broadcast later, on the host


def test_tails_refuse_an_infinite_null_val_and_keep_their_finite_contracts():
    from step_amd import TSFormer
    from step_amd.step_loss import train_tail
    x = torch.zeros(2, 12, 3, 1)
    m = TSFormer(12, 1, 96, 4, 4, 0.1, 4, 0.75, 4, 1, mode="pre-train")
    for nv in (float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            m.pretrain_tail(torch.zeros(2, 48, 3, 1), nv)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # None, "only NaN labels are masked", passes the host checks
        m.pretrain_tail(torch.zeros(2, 48, 3, 1), None)
    t = torch.full((2, 4, 4), 0.5)
    with pytest.raises(ValueError, match="f32 device tensors"):          # CPU tensors are refused first, whatever the null value
        train_tail(x, x, t, t, 1.0, null_val=NAN)
