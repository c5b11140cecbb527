"""Reference side of the per-node evaluation tests (tests/test_eval_per_node_host.py, tests/test_gpu_eval_per_node.py): the reference's
OWN masked_mae / masked_rmse / masked_mape (basicts/metrics/{mae,rmse,mape}.py, located and loaded as tools/make_eval_metrics_golden.py
does) applied, for EVERY node n, to the rescaled slices [:, h, n] of every horizon and [:, :, n] of all of them.  Inputs are normalised;
the metrics are taken on x * scale + shift (re_standard_transform), in f32 as the runner does.  Runs on the CPU; needs the reference
checkout.  Writes tests/golden/eval_per_node_cases.npz (about 80 KB).

    python tools/make_eval_per_node_golden.py

Keys, per case c in `cases`: c.pred f32 [B, H, N]; c.real f32 [B, H, N, C] with the label in channel c.channel; c.scale, c.shift f32
(scalars, or [N] for a per-node scaler: mean / std of shape [1, N, 1]); c.null_val f64 (0.0 or NaN); c.split (batch sizes of a split
feed); c.null_node: the node whose labels are ALL null (its expected rows are all 0), -1 for none; c.expected f64 [N, H + 1, 3]: MAE,
RMSE, MAPE of node n at horizon h, in row H over all horizons (every entry a float32 result of the reference, widened).

Cases (the smallest shapes at which the kernel can go wrong):
  a      [7, 12, 5]   unscaled; labels one float32 step either side of 5e-5 and of 1e-4 (and on them), NaN labels, NaN predictions on a
                      null and on counted labels
  b      [7, 12, 5]   the label as channel 1 of [B, H, N, 3], std 38.25 / mean 207.227: a quarter of the labels are the image of a raw
                      0.0, a run of adjacent float32 labels crosses both thresholds after rescaling
  n257   [9, 2, 257]  one node beyond a 256-thread workgroup
  one    [1, 1, 1]    one window, one node -- which is the null node: all 0
  live   [1, 1, 1]    one window, one node, counted
  h64    [2, 64, 3]   the largest H
  nan    [7, 12, 5]   null_val = NaN (the reference's default branch): NaN labels are the null ones, 0.0 labels count for MAE / RMSE
  pn     [7, 12, 5]   per-node scaler, label as channel 2 of 3
In every case but `live` ONE node has every label null; every other (node, horizon) keeps at least one label counted by the MAE / RMSE
mask and one counted by the MAPE mask (asserted below), so no other cell of the table is an accident of 0 / 0.  (`one` is the
one-window, one-node case with its node as the null node; `live` is the same shape with a counted label, so that the shape is also
checked on numbers other than 0.)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_eval_metrics_golden import reference_metrics          # noqa: E402

F = np.float32


def labels(rng, B, H, N, p_null):
    """raw labels in 5 .. 60, a share p_null of them 0.0, at least one window of every (horizon, node) kept away from 0"""
    raw = rng.uniform(5.0, 60.0, size=(B, H, N)).astype(F)
    keep = rng.integers(0, B, size=(H, N))
    null = rng.random(raw.shape) < p_null
    null[keep, np.arange(H)[:, None], np.arange(N)[None, :]] = False
    raw[null] = 0.0
    return raw, keep


def case_a(rng):
    B, H, N = 7, 12, 5
    real, keep = labels(rng, B, H, N, 0.25)
    pred = (real + rng.normal(0.0, 4.0, size=real.shape)).astype(F)
    lo, hi = F(5e-5), F(1e-4)
    edge = [np.nextafter(lo, F(0)), lo, np.nextafter(lo, F(1)), np.nextafter(hi, F(0)), hi, np.nextafter(hi, F(1)), F(3e-5), F(8e-5)]
    spots = [(b, h, n) for h in (0, 5) for n in (0, 1, 2, 4) for b in range(B) if b != keep[h, n]][:2 * len(edge)]
    for (b, h, n), v in zip(spots, edge + [-x for x in edge]):
        real[b, h, n] = v
    free = [(b, 1, n) for n in (0, 1, 2) for b in range(B) if b != keep[1, n]]
    real[free[0]] = np.nan                                   # a NaN label next to a finite null_val: counted, its terms add 0
    real[free[1]] = 0.0
    pred[free[1]] = np.nan                                   # a NaN prediction on a null label
    real[free[2]] = 17.5
    pred[free[2]] = np.nan                                   # ... on a counted label
    b, h, n = 6, 3, 4
    real[b, h, n], pred[b, h, n] = 23.25, np.nan             # ... in the last window (the batch of one of the split)
    real[:, :, 3] = 0.0
    pred[1, 2, 3] = np.nan
    return dict(pred=pred, real=real[..., None], channel=0, scale=F(1.0), shift=F(0.0), null_val=0.0, null_node=3, split=[3, 3, 1])


def case_b(rng):
    B, H, N = 7, 12, 5
    scale, shift = F(38.25), F(207.227)
    raw, keep = labels(rng, B, H, N, 0.25)
    raw = raw * F(10.0)
    y = ((raw - shift) / scale).astype(F)
    # adjacent float32 labels around the image of a raw 0.0: after rescaling they step through 0 .. 2e-4 and cross both thresholds
    at = F(-shift / scale)
    run = [at]
    for _ in range(12):
        run.append(np.nextafter(run[-1], F(0)))
    run += [np.nextafter(at, F(-10)), np.nextafter(np.nextafter(at, F(-10)), F(-10))]
    spots = [(b, h, n) for h in (2, 7, 9) for n in (0, 2, 3, 4) for b in range(B) if b != keep[h, n]][:len(run)]
    for spot, v in zip(spots, run):
        y[spot] = v
    y[:, :, 1] = at                                          # the null node: the image of a raw 0.0 (comes back within 5e-5 of 0)
    pred = (y + rng.normal(0.0, 0.2, size=y.shape)).astype(F)
    real = rng.normal(size=(B, H, N, 3)).astype(F)
    real[..., 1] = y
    return dict(pred=pred, real=real, channel=1, scale=scale, shift=shift, null_val=0.0, null_node=1, split=[3, 3, 1])


def case_plain(rng, B, H, N, null_node, split, p_null):
    real, _ = labels(rng, B, H, N, p_null)
    pred = (real + rng.normal(0.0, 3.0, size=real.shape)).astype(F)
    if null_node >= 0:
        real[:, :, null_node] = 0.0
    return dict(pred=pred, real=real[..., None], channel=0, scale=F(1.0), shift=F(0.0), null_val=0.0, null_node=null_node, split=split)


def case_nan(rng):
    B, H, N = 7, 12, 5
    real, keep = labels(rng, B, H, N, 0.2)                  # the 0.0 labels count for MAE / RMSE here, not for MAPE
    miss = rng.random(real.shape) < 0.2
    miss[keep, np.arange(H)[:, None], np.arange(N)[None, :]] = False
    real[miss] = np.nan
    pred = (real + rng.normal(0.0, 4.0, size=real.shape)).astype(F)
    pred[np.isnan(pred)] = 30.0
    free = [(b, 4, 0) for b in range(B) if b != keep[4, 0]]
    pred[free[0]] = np.nan                                   # a NaN prediction on whatever label is there
    real[:, :, 2] = np.nan
    scale, shift = F(1.5), F(-2.0)
    y = ((real - shift) / scale).astype(F)
    return dict(pred=((pred - shift) / scale).astype(F), real=y[..., None], channel=0, scale=scale, shift=shift, null_val=float("nan"),
                null_node=2, split=[3, 3, 1])


def case_pn(rng):
    B, H, N = 7, 12, 5
    scale = rng.uniform(5.0, 60.0, size=N).astype(F)
    shift = rng.uniform(50.0, 300.0, size=N).astype(F)
    raw, _ = labels(rng, B, H, N, 0.25)
    raw = raw * F(8.0)
    raw[:, :, 0] = 0.0
    y = ((raw - shift) / scale).astype(F)
    pred = (y + rng.normal(0.0, 0.2, size=y.shape)).astype(F)
    real = rng.normal(size=(B, H, N, 3)).astype(F)
    real[..., 2] = y
    return dict(pred=pred, real=real, channel=2, scale=scale, shift=shift, null_val=0.0, null_node=0, split=[3, 3, 1])


def record(fns, c):
    scale, shift = torch.from_numpy(np.asarray(c["scale"])), torch.from_numpy(np.asarray(c["shift"]))
    if scale.dim() == 1:          # mean / std of shape [1, N, 1] against [B, H, N, 1]: re_standard_transform's broadcast
        p = (torch.from_numpy(c["pred"])[..., None] * scale.view(1, -1, 1) + shift.view(1, -1, 1))[..., 0]
        y = (torch.from_numpy(c["real"][..., c["channel"]])[..., None] * scale.view(1, -1, 1) + shift.view(1, -1, 1))[..., 0]
    else:
        p = torch.from_numpy(c["pred"]) * scale + shift          # data * std + mean
        y = torch.from_numpy(c["real"][..., c["channel"]]) * scale + shift
    assert p.dtype == torch.float32 and y.dtype == torch.float32
    B, H, N = p.shape
    nv = c["null_val"]

    def three(a, b):
        return [float(f(a, b, null_val=nv).item()) for f in fns]
    out = np.zeros((N, H + 1, 3), dtype=np.float64)
    for n in range(N):
        for h in range(H):
            out[n, h] = three(p[:, h, n], y[:, h, n])
        out[n, H] = three(p[:, :, n], y[:, :, n])
    # the cells that are 0 are the null node's, and only those
    counted = ~torch.isnan(y) if nv != nv else ~torch.isclose(y, torch.full_like(y, nv), atol=5e-5, rtol=0.0)
    y0 = torch.where(torch.abs(y) < 1e-4, torch.zeros_like(y), y)
    counted0 = ~torch.isclose(y0, torch.zeros_like(y0), atol=5e-5, rtol=0.0)
    for mask in (counted, counted0):
        per = mask.sum(dim=0)          # [H, N]
        for n in range(N):
            if n != c["null_node"]:
                assert (per[:, n] >= 1).all(), (n, per[:, n])
            elif mask is counted or nv == nv:          # (MAPE's own null value is 0: a NaN label is counted there, its NaN term adds 0)
                assert (per[:, n] == 0).all(), (n, per[:, n])
    if c["null_node"] >= 0:
        assert (out[c["null_node"]] == 0.0).all()
    assert np.isfinite(out).all()
    return out, float(counted.float().mean()), float(counted0.float().mean())


def main():
    fns = reference_metrics()
    rng = np.random.default_rng(20261021)
    cases = {"a": case_a(rng), "b": case_b(rng), "n257": case_plain(rng, 9, 2, 257, 200, [3, 3, 3], 0.25),
             "one": case_plain(rng, 1, 1, 1, 0, [1], 0.0), "live": case_plain(rng, 1, 1, 1, -1, [1], 0.0),
             "h64": case_plain(rng, 2, 64, 3, 1, [1, 1], 0.0), "nan": case_nan(rng), "pn": case_pn(rng)}
    out = {"cases": np.array(sorted(cases))}
    for name, c in cases.items():
        for x in (c["pred"], c["real"]):
            assert x.dtype == F and np.isfinite(x[~np.isnan(x)]).all()          # no infinite values
        assert sum(c["split"]) == c["pred"].shape[0]
        expected, share, share0 = record(fns, c)
        out.update({f"{name}.pred": c["pred"], f"{name}.real": c["real"], f"{name}.channel": np.int64(c["channel"]),
                    f"{name}.scale": np.asarray(c["scale"], dtype=F), f"{name}.shift": np.asarray(c["shift"], dtype=F),
                    f"{name}.null_val": np.float64(c["null_val"]), f"{name}.null_node": np.int64(c["null_node"]),
                    f"{name}.split": np.array(c["split"], dtype=np.int64), f"{name}.expected": expected})
        print(f"{name}: {c['pred'].shape}, counted share {share:.2f} (MAPE {share0:.2f}), overall of node 0 {expected[0, -1]}")
    path = os.path.join(ROOT, "tests", "golden", "eval_per_node_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
