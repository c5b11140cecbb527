"""Evaluation metrics, host side (no GPU): the size query and the new symbols, what the accumulator class refuses before it touches a
device, the recorded fixture against a float64 restatement of the semantics that include/step_hip.h promises (so the fixture and the
header say the same thing), and the source rule of step_amd/evaluate.py: one device-to-host copy per pass.  The kernel itself:
tests/test_gpu_eval_metrics.py."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "eval_metrics_cases.npz")


def test_accumulator_size_query_and_symbols():
    from step_amd import _lib
    lib = _lib.lib()
    assert lib.step_eval_metrics_acc_doubles(12) > 0
    assert lib.step_eval_metrics_acc_doubles(0) == 0 and lib.step_eval_metrics_acc_doubles(65) == 0
    assert lib.step_eval_metrics_acc_doubles(-3) == 0
    assert 0 < lib.step_eval_metrics_acc_doubles(1) < lib.step_eval_metrics_acc_doubles(64)          # five sums per horizon at least
    assert lib.step_eval_metrics_acc_doubles(64) - lib.step_eval_metrics_acc_doubles(63) >= 5
    for name in ("step_eval_metrics_accumulate", "step_eval_metrics_finish"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.step_abi_version() == 10


def test_entry_points_reject_bad_sizes_before_touching_the_device():
    """beyond the all-NULL call of tests/test_abi_and_host.py: non-NULL pointers with H = 65, a zero stride, a negative size"""
    import ctypes
    from step_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(sb=60, sh=5, sn=1, B=2, H=12, N=5)

    def accumulate(**kw):
        a = dict(good, **kw)
        return lib.step_eval_metrics_accumulate(p, a["sb"], a["sh"], a["sn"], p, a["sb"], a["sh"], a["sn"], a["B"], a["H"], a["N"], 1.0, 0.0,
                                                0.0, p, None)
    for bad, word in ((dict(H=65), "H = 65"), (dict(sn=0), "strides"), (dict(sh=-5), "strides"), (dict(B=-1), "positive"),
                      (dict(N=0), "positive")):
        assert accumulate(**bad) == 1, bad
        assert word in lib.step_last_error().decode(), (bad, lib.step_last_error())
    assert lib.step_eval_metrics_accumulate(p, 60, 5, 1, p, 60, 5, 1, 2, 12, 5, 1.0, 0.0, 0.0, None, None) == 1
    for H in (0, 65):
        assert lib.step_eval_metrics_finish(p, H, p, None) == 1
        assert f"H = {H}" in lib.step_last_error().decode()
    assert lib.step_eval_metrics_finish(p, 12, None, None) == 1


def test_python_surface_refuses_what_cannot_run():
    import step_amd
    from step_amd.evaluate import EvalMetrics, EvalResult, _scale_shift
    assert step_amd.EvalMetrics is EvalMetrics and step_amd.EvalResult is EvalResult
    assert callable(step_amd.STEP.evaluate)
    for H in (0, 65):
        with pytest.raises(ValueError, match="horizons"):
            EvalMetrics(horizons=H, device="cuda")          # refused by the size query, before any allocation
    with pytest.raises(ValueError, match="no CPU fallback"):
        EvalMetrics(horizons=12, device="cpu")
    assert _scale_shift(None) is None
    assert _scale_shift((207.0, 38.5)) == (38.5, 207.0)          # (mean, std) -> (scale, shift)
    assert _scale_shift({"mean": 1.5, "std": 2.0}) == (2.0, 1.5)
    assert _scale_shift({"func": "re_standard_transform", "args": {"mean": 1.5, "std": 2.0}}) == (2.0, 1.5)
    with pytest.raises(ValueError, match="finite"):
        _scale_shift((float("nan"), 1.0))


# ---------------------------------------------------------------------------------------------- the fixture says what the header says
def _three(p, y, null_val):
    """include/step_hip.h, "evaluation metrics", in float64 over f32 terms"""
    p, y = p.reshape(-1), y.reshape(-1)
    with np.errstate(all="ignore"):
        m = ~np.isnan(y) if np.isnan(null_val) else ~(np.abs(y - np.float32(null_val)) <= np.float32(5e-5))
        d = (p - y).astype(np.float32)
        cnt = m.sum()
        mae = np.nansum(np.abs(d)[m].astype(np.float64)) / cnt if cnt else 0.0
        mse = np.nansum((d * d)[m].astype(np.float64)) / cnt if cnt else 0.0
        y0 = np.where(np.abs(y) < np.float32(1e-4), np.float32(0.0), y)
        m0 = ~(np.abs(y0) <= np.float32(5e-5))
        ape = np.abs(np.abs(p - y0) / y0).astype(np.float32)
        mape = np.nansum(ape[m0].astype(np.float64)) / m0.sum() if m0.sum() else 0.0
    return [mae, np.sqrt(mse), mape]


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(got - want) <= np.where(want == 0.0, 1e-6, 1e-5 * np.abs(want))))


def test_fixture_holds_the_cases_and_agrees_with_the_stated_semantics():
    z = np.load(FIXTURE, allow_pickle=False)
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert sorted(z["cases"].tolist()) == ["a", "b", "c1", "c2"]
    assert z["a.pred"].shape == (7, 12, 5) and z["b.pred"].shape == (3, 12, 300) and z["b.real"].shape == (3, 12, 300, 3)
    assert int(z["b.channel"]) == 1 and z["c1.pred"].shape == (1, 1, 1) and z["c2.pred"].shape == (2, 1, 70)
    a_real = z["a.real"][..., 0]
    assert (a_real[:, 4, :] == 0).all() and np.isnan(a_real).sum() == 1 and np.isnan(z["a.pred"]).sum() == 2
    assert 0.25 < (a_real == 0).mean() < 0.40 and (a_real == np.float32(3e-5)).any() and (a_real == np.float32(8e-5)).any()
    assert float(z["b.scale"]) != 1.0 and float(z["b.shift"]) != 0.0
    for name in z["cases"].tolist():
        pred, real = z[f"{name}.pred"], z[f"{name}.real"][..., int(z[f"{name}.channel"])]
        assert pred.dtype == np.float32 and real.dtype == np.float32
        assert not np.isinf(pred).any() and not np.isinf(real).any()
        scale, shift = z[f"{name}.scale"], z[f"{name}.shift"]
        p, y = pred * scale + shift, real * scale + shift          # float32: a rounded multiply, then a rounded add
        assert p.dtype == np.float32
        for tag, null_val in (("zero", 0.0), ("nan", float("nan"))):
            per_h = [_three(p[:, h], y[:, h], null_val) for h in range(p.shape[1])]
            assert _close(per_h, z[f"{name}.{tag}.per_horizon"]), (name, tag)
            assert _close(_three(p, y, null_val), z[f"{name}.{tag}.overall"]), (name, tag)
            at, rows = 0, []
            for n in z[f"{name}.split"].tolist():
                rows.append(_three(p[at:at + n], y[at:at + n], null_val))
                at += n
            assert _close(np.mean(rows, axis=0), z[f"{name}.{tag}.batch_mean_split"]), (name, tag)
    assert (z["a.zero.per_horizon"][4] == 0).all()          # the all-null horizon: a count of 0 gives 0


# ---------------------------------------------------------------------------------------------- one device-to-host copy per pass
def test_evaluate_module_reads_the_device_once_per_pass():
    src = open(os.path.join(ROOT, "step_amd", "evaluate.py")).read()
    code = re.sub(r'""".*?"""', "", src, flags=re.S)
    code = "\n".join(line.split("#")[0] for line in code.splitlines())
    reads = re.findall(r"\.(?:cpu|item|tolist|numpy|synchronize)\(", code) + re.findall(r"\.to\(\s*[\"']cpu", code)
    assert reads == [".cpu(", ".numpy("], reads          # `self._out.cpu().numpy()`, nothing else
    result_body = code.split("def result(")[1].split("\ndef ")[0]
    assert ".cpu(" in result_body
    assert "float(" not in code.split("def update(")[1].split("def result(")[0]          # update() converts no tensor to a host number
