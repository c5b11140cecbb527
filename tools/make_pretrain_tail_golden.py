"""Reference side of the pre-training tail tests (tests/test_gpu_pretrain_tail.py, tests/test_pretrain_tail_host.py): the reference's OWN
re_standard_transform (basicts/data/transform.py) and masked_mae / masked_rmse / masked_mape (basicts/metrics/{mae,rmse,mape}.py), loaded
as tools/make_train_tail_golden.py loads them, on the masked tokens of small hand-built cases, as the runner evaluates them in a
pre-training iteration (basicts/runners/base_tsf_runner.py:237-254): rescale, loss, backward, three metrics -- all in f32 on the CPU.
The masked tokens are selected as step/step_arch/tsformer/tsformer.py:152-158 selects them, restated on the decoder's output r [S, P, 12]
and the packed series [S, P * 12] as index arithmetic: the reconstruction of masked token j is row Pu + j of r, its label is patch
mk[j] of the series.  Needs the reference checkout (oracle/reference_loader.py).  Writes tests/golden/pretrain_tail_cases.npz.

    python tools/make_pretrain_tail_golden.py

Keys, per case c in `cases`: c.r f32 [S, P, 12] (normalised); c.series f32 [S, P * 12]; c.mk int32 [Pm]; c.Pu, c.B, c.N int64; c.scale,
c.shift f32; c.loss f32; c.metrics f32 [3] (MAE, RMSE, MAPE); c.dr f32 [S, P, 12], the gradient w.r.t. the NORMALISED r (NaN where r
is: the reference's gradient of a NaN term is NaN, the kernel's is defined as 0)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "pretrain_tail_cases.npz")


def reference_functions():
    """-> (re_standard_transform, [masked_mae, masked_rmse, masked_mape]) of the reference"""
    spec = importlib.util.spec_from_file_location("make_train_tail_golden", os.path.join(ROOT, "tools", "make_train_tail_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, rescale, metrics = tool.reference_functions()
    return rescale, metrics


def masked_labels(rng, S, Pm, scale, shift):
    """labels of the masked tokens [S, Pm, 12] as labels_and_pred of tools/make_train_tail_golden.py builds them: the normalised image of a
    raw series in which a fifth of the values are exactly 0 and two dozen sit next to the 5e-5 / 1e-4 thresholds"""
    raw = rng.uniform(20.0, 600.0, size=(S, Pm, 12)).astype(np.float32)
    raw[rng.random(raw.shape) < 0.2] = 0.0
    near = rng.permutation(raw.size)[:24]
    raw.reshape(-1)[near] = np.repeat(np.float32([2e-5, 4e-5, 5e-5, 6e-5, 9e-5, 1.2e-4]), 4)
    return ((raw - np.float32(shift)) / np.float32(scale)).astype(np.float32)


def tensors(rng, S, P, mk, scale, shift, noise, y=None):
    """-> (r [S, P, 12], series [S, P * 12]): the labels at the patches mk, other data elsewhere; r = label + noise in the masked rows"""
    Pm = len(mk)
    Pu = P - Pm
    if y is None:
        y = masked_labels(rng, S, Pm, scale, shift)
    series = rng.normal(0.0, 1.0, size=(S, P, 12)).astype(np.float32)
    series[:, mk, :] = y
    r = rng.normal(0.0, 1.0, size=(S, P, 12)).astype(np.float32)
    r[:, Pu:, :] = (y + rng.normal(0.0, noise / scale, size=y.shape)).astype(np.float32)
    return r, series.reshape(S, P * 12)


def build_cases():
    rng = np.random.default_rng(20241019)
    cases = {}

    def case(B, N, P, mk, scale, shift, noise):
        r, series = tensors(rng, B * N, P, mk, scale, shift, noise)
        return dict(r=r, series=series, mk=np.array(mk, dtype=np.int32), Pu=P - len(mk), B=B, N=N, scale=scale, shift=shift)
    cases["a"] = case(1, 3, 4, [3, 0, 2], 1.0, 0.0, 4.0)
    sorted_mk = lambda P, Pm: sorted(rng.permutation(P)[:Pm].tolist())
    cases["b"] = case(2, 5, 14, sorted_mk(14, 10), 38.25, 207.227, 8.0)
    cases["c"] = case(2, 37, 28, sorted_mk(28, 21), 150.0, 200.0, 20.0)
    b = cases["b"]
    # d: case b with every label of a masked token null
    sd = b["series"].reshape(10, 14, 12).copy()
    sd[:, b["mk"], :] = ((np.float32(0.0) - np.float32(b["shift"])) / np.float32(b["scale"])).astype(np.float32)
    cases["d"] = dict(b, series=sd.reshape(10, 14 * 12))
    # e: case b with one NaN in a masked-token row of r, on a counted label; e_un: one NaN in an unmasked row
    yb = b["series"].reshape(10, 14, 12)[:, b["mk"], :] * np.float32(b["scale"]) + np.float32(b["shift"])
    s, j, i = np.argwhere(np.abs(yb) > 1.0)[7]
    re = b["r"].copy()
    re[s, b["Pu"] + j, i] = np.nan
    cases["e"] = dict(b, r=re)
    ru = b["r"].copy()
    ru[4, 1, 5] = np.nan
    assert b["Pu"] > 1
    cases["e_un"] = dict(b, r=ru)
    return cases


def select(case, r, series):
    """tsformer.py:152-158 on r / series: -> (reconstruction, label) of the masked tokens, [B, Pm * 12, N] each"""
    B, N, Pu = int(case["B"]), int(case["N"]), int(case["Pu"])
    P = r.shape[1]
    recon = r.view(B, N, P, 12)[:, :, Pu:, :].reshape(B, N, -1).transpose(1, 2)
    label = series.view(B, N, P, 12)[:, :, torch.from_numpy(case["mk"]).long(), :].reshape(B, N, -1).transpose(1, 2)
    return recon, label


def record(fns, case):
    rescale, metrics = fns
    scale, shift = float(case["scale"]), float(case["shift"])
    r = torch.from_numpy(case["r"]).clone().requires_grad_(True)
    recon, label = select(case, r, torch.from_numpy(case["series"]))
    p, y = rescale(recon, mean=shift, std=scale), rescale(label, mean=shift, std=scale)
    loss = metrics[0](p, y, null_val=0.0)
    dr, = torch.autograd.grad(loss, [r])
    return {"loss": np.float32(loss.item()), "metrics": np.array([f(p.detach(), y, null_val=0.0).item() for f in metrics], dtype=np.float32),
            "dr": dr.numpy().copy()}


def compute():
    """-> the fixture's content as a dict of numpy arrays"""
    fns = reference_functions()
    cases = build_cases()
    out = {"cases": np.array(sorted(cases))}
    for name, case in cases.items():
        _, label = select(case, torch.from_numpy(case["r"]), torch.from_numpy(case["series"]))
        y = label * float(case["scale"]) + float(case["shift"])
        share = float((~torch.isclose(y, torch.zeros_like(y), atol=5e-5, rtol=0.0)).float().mean())
        assert share == 0.0 if name == "d" else share >= 0.5, (name, share)
        for key in ("r", "series", "mk"):
            out[f"{name}.{key}"] = case[key]
        for key in ("Pu", "B", "N"):
            out[f"{name}.{key}"] = np.int64(case[key])
        for key in ("scale", "shift"):
            out[f"{name}.{key}"] = np.float32(case[key])
        for key, v in record(fns, case).items():
            finite = np.isfinite(v) | np.isnan(case["r"]) if key == "dr" else np.isfinite(v)
            assert finite.all(), (name, key)
            out[f"{name}.{key}"] = v
    return out


def main():
    out = compute()
    for name in out["cases"]:
        print(name, out[f"{name}.r"].shape, float(out[f"{name}.loss"]), out[f"{name}.metrics"].tolist())
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
