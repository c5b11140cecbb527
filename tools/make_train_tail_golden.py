"""Reference side of the training-tail tests (tests/test_gpu_train_tail.py, tests/test_train_tail_host.py): the reference's OWN
step_loss (step/step_loss/step_loss.py, loaded the way tools/make_golden.py loads the reference), re_standard_transform
(basicts/data/transform.py) and masked_mae / masked_rmse / masked_mape (basicts/metrics/{mae,rmse,mape}.py, loaded by file as in
tools/make_eval_metrics_golden.py) on the first k horizon steps of small hand-built cases, as the runner evaluates them under curriculum
learning (basicts/runners/base_tsf_runner.py:237-254): rescale, slice [:, :k], loss, backward, three metrics -- all in f32 on the CPU.
Needs the reference checkout (oracle/reference_loader.py).  Writes tests/golden/train_tail_cases.npz.

    python tools/make_train_tail_golden.py

Keys, per case c in `cases`: c.pred f32 [B, 12, N] (normalised); c.real f32 [B, 12, N, C] with the label in channel 0; c.scale, c.shift,
c.coef f32; c.theta, c.prior f32 [B, 16, 16]; c.dtheta f32 [B, 16, 16] (it does not depend on k); and for k in `ks`: c.k.loss f32,
c.k.metrics f32 [3] (MAE, RMSE, MAPE), c.k.dpred f32 [B, 12, N] (the gradient w.r.t. the NORMALISED prediction, zero on the excluded
horizons) -- the last only where no included prediction is NaN."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.reference_loader import reference_root          # noqa: E402

KS = (1, 5, 11, 12)
H = 12
PATH = os.path.join(ROOT, "tests", "golden", "train_tail_cases.npz")


def _by_file(root, name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_functions():
    """-> (step_loss, re_standard_transform, [masked_mae, masked_rmse, masked_mape]) of the reference"""
    root = reference_root()
    assert root, "the reference checkout is needed to record this fixture"
    metrics = [getattr(_by_file(root, "ref_metric_" + mod, "basicts", "metrics", mod + ".py"), name)
               for mod, name in (("mae", "masked_mae"), ("rmse", "masked_rmse"), ("mape", "masked_mape"))]
    # basicts/__init__ pulls in the launcher and the runners (easytorch): stub the package shells, as tools/make_golden.py does; the
    # scaler registry of basicts/data/registry.py is easytorch's Registry, for which tests/_shims has a stand-in
    shims = os.path.join(ROOT, "tests", "_shims")
    if shims not in sys.path:
        sys.path.append(shims)
    saved = {k: sys.modules.get(k) for k in ("basicts", "step")}
    for pkg in ("basicts", "step"):
        shell = types.ModuleType(pkg)
        shell.__path__ = [os.path.join(root, pkg)]
        sys.modules[pkg] = shell
    try:
        from step.step_loss.step_loss import step_loss
        transform = _by_file(root, "basicts.data.transform", "basicts", "data", "transform.py")
    finally:
        for k, v in saved.items():
            for name in [n for n in sys.modules if n == k or n.startswith(k + ".")]:
                del sys.modules[name]
            if v is not None:
                sys.modules[k] = v
    return step_loss, transform.re_standard_transform, metrics


def labels_and_pred(rng, B, N, C, scale, shift, noise):
    """labels as in case_b of tools/make_eval_metrics_golden.py: the normalised image of a raw series in which a fifth of the values are
    exactly 0 and two dozen sit next to the 5e-5 / 1e-4 thresholds; the other channels hold small integers"""
    raw = rng.uniform(20.0, 600.0, size=(B, H, N)).astype(np.float32)
    raw[rng.random(raw.shape) < 0.2] = 0.0
    near = rng.permutation(raw.size)[:24]
    raw.reshape(-1)[near] = np.repeat(np.float32([2e-5, 4e-5, 5e-5, 6e-5, 9e-5, 1.2e-4]), 4)
    y = ((raw - np.float32(shift)) / np.float32(scale)).astype(np.float32)
    real = rng.integers(-3, 4, size=(B, H, N, C)).astype(np.float32)
    real[..., 0] = y
    pred = (y + rng.normal(0.0, noise / scale, size=y.shape)).astype(np.float32)
    return pred, real


def graph(rng, B):
    theta = np.clip(rng.random((B, 16, 16)), 1e-4, 1 - 1e-4).astype(np.float32)
    prior = (rng.random((B, 16, 16)) < 0.1).astype(np.float32)
    return theta, prior


def build_cases():
    rng = np.random.default_rng(20241018)
    cases = {}
    pa, ra = labels_and_pred(rng, 3, 5, 1, 1.0, 0.0, 4.0)
    ta = graph(rng, 3)
    cases["a"] = dict(pred=pa, real=ra, scale=1.0, shift=0.0, coef=1.0, theta=ta[0], prior=ta[1])
    pb, rb = labels_and_pred(rng, 2, 70, 3, 38.25, 207.227, 8.0)
    tb = graph(rng, 2)
    cases["b"] = dict(pred=pb, real=rb, scale=38.25, shift=207.227, coef=0.5, theta=tb[0], prior=tb[1])
    pc, rc = labels_and_pred(rng, 4, 307, 3, 150.0, 200.0, 20.0)
    tc = graph(rng, 4)
    cases["c"] = dict(pred=pc, real=rc, scale=150.0, shift=200.0, coef=0.25, theta=tc[0], prior=tc[1])
    # d: case a with every label of horizons 0..4 null and none of horizons 5..11
    rd = ra.copy()
    rd[:, :5, :, 0] = 0.0
    late = rd[:, 5:, :, 0]
    late[np.abs(late) < 1.0] = 37.5
    cases["d"] = dict(cases["a"], real=rd)
    # e: case a with one NaN prediction, in the last horizon (excluded for k < 12) and, separately, in the first (always included)
    for name, h in (("e11", 11), ("e0", 0)):
        pe = pa.copy()
        b, n = np.argwhere(np.abs(ra[:, h, :, 0]) > 1.0)[0]          # on a counted label
        pe[b, h, n] = np.nan
        cases[name] = dict(cases["a"], pred=pe)
    return cases


def record(fns, case):
    step_loss, rescale, metrics = fns
    scale, shift = float(case["scale"]), float(case["shift"])
    real = torch.from_numpy(case["real"][..., :1])
    out = {}
    for k in KS:
        pred = torch.from_numpy(case["pred"])[..., None].clone().requires_grad_(True)
        theta = torch.from_numpy(case["theta"]).clone().requires_grad_(True)
        p = rescale(pred, mean=shift, std=scale)[:, :k, :, :]
        y = rescale(real, mean=shift, std=scale)[:, :k, :, :]
        loss = step_loss(p, y, theta, torch.from_numpy(case["prior"]), float(case["coef"]), null_val=0.0)
        dpred, dtheta = torch.autograd.grad(loss, [pred, theta])
        out[f"{k}.loss"] = np.float32(loss.item())
        out[f"{k}.metrics"] = np.array([f(p.detach(), y, null_val=0.0).item() for f in metrics], dtype=np.float32)
        if not torch.isnan(pred[:, :k]).any():
            out[f"{k}.dpred"] = dpred[..., 0].numpy().copy()
        if "dtheta" in out:
            assert np.array_equal(out["dtheta"], dtheta.numpy())
        out["dtheta"] = dtheta.numpy().copy()
    return out


def compute():
    """-> the fixture's content as a dict of numpy arrays"""
    fns = reference_functions()
    cases = build_cases()
    out = {"cases": np.array(sorted(cases)), "ks": np.array(KS, dtype=np.int64)}
    for name, case in cases.items():
        y = torch.from_numpy(case["real"][..., 0]) * float(case["scale"]) + float(case["shift"])
        kept = ~torch.isclose(y, torch.zeros_like(y), atol=5e-5, rtol=0.0)
        for k in KS:
            share = float(kept[:, :k].float().mean())
            if name == "d":
                assert (share == 0.0) == (k <= 5), (k, share)
            else:
                assert share >= 0.5, (name, k, share)
        for key in ("pred", "real", "theta", "prior"):
            out[f"{name}.{key}"] = case[key]
        for key in ("scale", "shift", "coef"):
            out[f"{name}.{key}"] = np.float32(case[key])
        for key, v in record(fns, case).items():
            assert np.isfinite(v).all(), (name, key)
            out[f"{name}.{key}"] = v
    return out


def main():
    out = compute()
    for name in out["cases"]:
        print(name, {k: (float(out[f"{name}.{k}.loss"]), out[f"{name}.{k}.metrics"].tolist()) for k in KS})
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
