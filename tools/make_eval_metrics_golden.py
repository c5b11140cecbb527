"""Reference side of the evaluation-metric tests (tests/test_gpu_eval_metrics.py): the reference's OWN masked_mae / masked_rmse /
masked_mape (basicts/metrics/{mae,rmse,mape}.py, loaded by file: the package's __init__ pulls in its whole runner stack) on small
hand-built cases, per horizon, over everything and as the mean over a split into batches, for null_val = 0.0 and NaN.  Inputs are
normalised; the metrics are taken on x * scale + shift (basicts/data/transform.py re_standard_transform), in f32 as the runner does.
Runs on the CPU; needs the reference checkout (oracle/reference_loader.py).  Writes tests/golden/eval_metrics_cases.npz (~170 KB).

    python tools/make_eval_metrics_golden.py

Keys, per case c in `cases`: c.pred f32 [B, H, N]; c.real f32 [B, H, N, C] with the label in channel c.channel; c.scale, c.shift f32;
c.split (batch sizes); and for tag in (zero, nan): c.tag.per_horizon f64 [H, 3], c.tag.overall [3], c.tag.batch_mean_split [3] (the
columns are MAE, RMSE, MAPE; every entry is a float32 result of the reference, widened)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.reference_loader import reference_root          # noqa: E402


def reference_metrics():
    root = reference_root()
    assert root, "the reference checkout is needed to record this fixture"
    fns = []
    for mod, name in (("mae", "masked_mae"), ("rmse", "masked_rmse"), ("mape", "masked_mape")):
        spec = importlib.util.spec_from_file_location("ref_metric_" + mod, os.path.join(root, "basicts", "metrics", mod + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        fns.append(getattr(m, name))
    return fns


def case_a(rng):
    """[7, 12, 5], unscaled: exactly 10 of the 35 labels of every horizon are 0.0 (horizon 4: all of them), labels at 3e-5 and 8e-5, one
    NaN label, two NaN predictions (one of them on a null label)"""
    B, H, N = 7, 12, 5
    real = rng.uniform(5.0, 60.0, size=(B, H, N)).astype(np.float32)
    for h in range(H):
        flat = rng.permutation(B * N)[:10]
        real[flat // N, h, flat % N] = 0.0
    real[:, 4, :] = 0.0
    pred = (real + rng.normal(0.0, 4.0, size=real.shape)).astype(np.float32)
    real[0, 0, 0], real[1, 0, 1] = 3e-5, 8e-5          # under and over the 5e-5 threshold (both under MAPE's 1e-4)
    real[2, 1, 2] = np.nan
    real[3, 2, 3] = 0.0
    pred[3, 2, 3] = np.nan                              # on a null label
    real[6, 3, 0] = 17.5
    pred[6, 3, 0] = np.nan                              # on a counted label, in the last window (the batch of one of the split)
    return pred, real[..., None], 0, 1.0, 0.0, [3, 3, 1]


def case_b(rng):
    """[3, 12, 300], the label as channel 1 of three, scaler std 38.25 / mean 207.227: a fifth of the labels are the normalised image
    of a raw 0.0 (they come back as 0 up to rounding), a few sit next to the 5e-5 threshold after rescaling"""
    B, H, N = 3, 12, 300
    scale, shift = np.float32(38.25), np.float32(207.227)
    raw = rng.uniform(20.0, 600.0, size=(B, H, N)).astype(np.float32)
    raw[rng.random(raw.shape) < 0.2] = 0.0
    near = rng.permutation(raw.size)[:24]
    raw.reshape(-1)[near] = np.repeat(np.float32([2e-5, 4e-5, 5e-5, 6e-5, 9e-5, 1.2e-4]), 4)
    y = ((raw - shift) / scale).astype(np.float32)
    real = rng.normal(size=(B, H, N, 3)).astype(np.float32)
    real[..., 1] = y
    pred = (y + rng.normal(0.0, 0.2, size=y.shape)).astype(np.float32)
    return pred, real, 1, float(scale), float(shift), [2, 1]


def case_small(rng, B, N, split):
    real = rng.uniform(1.0, 9.0, size=(B, 1, N)).astype(np.float32)
    pred = (real + rng.normal(0.0, 0.5, size=real.shape)).astype(np.float32)
    return pred, real[..., None], 0, 1.0, 0.0, split


def record(fns, pred, real, channel, scale, shift, split, null_val):
    p = torch.from_numpy(pred) * scale + shift          # re_standard_transform: data * std + mean
    y = torch.from_numpy(real[..., channel]) * scale + shift

    def three(a, b):
        return [float(f(a, b, null_val=null_val).item()) for f in fns]
    per_h = np.array([three(p[:, h, :], y[:, h, :]) for h in range(p.shape[1])], dtype=np.float64)
    overall = np.array(three(p, y), dtype=np.float64)
    at, rows = 0, []
    for n in split:
        rows.append(three(p[at:at + n], y[at:at + n]))
        at += n
    assert at == p.shape[0]
    return per_h, overall, np.mean(np.array(rows, dtype=np.float64), axis=0)


def main():
    fns = reference_metrics()
    rng = np.random.default_rng(20240607)
    cases = {"a": case_a(rng), "b": case_b(rng), "c1": case_small(rng, 1, 1, [1]), "c2": case_small(rng, 2, 70, [1, 1])}
    out = {"cases": np.array(sorted(cases))}
    for name, (pred, real, channel, scale, shift, split) in cases.items():
        assert np.isfinite(pred[~np.isnan(pred)]).all() and np.isfinite(real[~np.isnan(real)]).all()          # no infinite values
        out.update({f"{name}.pred": pred, f"{name}.real": real, f"{name}.channel": np.int64(channel), f"{name}.scale": np.float32(scale),
                    f"{name}.shift": np.float32(shift), f"{name}.split": np.array(split, dtype=np.int64)})
        y = torch.from_numpy(real[..., channel]) * scale + shift
        kept = ~torch.isclose(y, torch.zeros_like(y), atol=5e-5, rtol=0.0)
        share = kept.float().mean(dim=(0, 2)).tolist()
        print(name, "unmasked share per horizon:", " ".join(f"{s:.2f}" for s in share))
        assert all(s >= 0.5 or (name == "a" and h == 4 and s == 0.0) for h, s in enumerate(share))
        for tag, null_val in (("zero", 0.0), ("nan", float("nan"))):
            per_h, overall, split_mean = record(fns, pred, real, channel, scale, shift, split, null_val)
            assert np.isfinite(per_h).all() and np.isfinite(overall).all() and np.isfinite(split_mean).all()
            out.update({f"{name}.{tag}.per_horizon": per_h, f"{name}.{tag}.overall": overall, f"{name}.{tag}.batch_mean_split": split_mean})
            print(name, tag, "overall", overall, "split mean", split_mean)
    path = os.path.join(ROOT, "tests", "golden", "eval_metrics_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
