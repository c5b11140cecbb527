"""Numpy restatement of the per-node evaluation metrics (csrc/eval_nodes.hip; include/step_hip.h, "per-node evaluation metrics"):
float32 element terms exactly as the kernel and the reference's masked_mae / masked_rmse / masked_mape take them, float64 sums.
Shared by tests/test_eval_per_node_host.py (against the reference's own numbers in tests/golden/eval_per_node_cases.npz) and
tests/test_gpu_eval_per_node.py (against the device).  No device, no library."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_per_node_cases.npz")
SUMS = ("S_abs", "S_sq", "cnt", "S_ape", "cnt0")


def load_fixture():
    z = np.load(FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_of(z, name):
    """-> dict(pred [B, H, N], real [B, H, N, C], channel, scale, shift (f32 scalars or [N]), null_val, null_node, split, expected)"""
    g = {k: z[f"{name}.{k}"] for k in ("pred", "real", "channel", "scale", "shift", "null_val", "null_node", "split", "expected")}
    g["channel"], g["null_node"], g["null_val"], g["split"] = int(g["channel"]), int(g["null_node"]), float(g["null_val"]), g["split"].tolist()
    return g


def rescaled(x, scale, shift):
    """x * scale + shift in float32 with two roundings (torch's `x * std + mean`); scale / shift scalars or [N] along the last axis"""
    x = np.asarray(x, dtype=np.float32)
    return (x * np.asarray(scale, dtype=np.float32)).astype(np.float32) + np.asarray(shift, dtype=np.float32)


def five_sums(pred, real, scale=1.0, shift=0.0, null_val=0.0):
    """pred, real f32 [B, H, N] normalised -> f64 [5, H, N]: S_abs, S_sq, cnt, S_ape, cnt0 per (horizon, node) over the B windows"""
    with np.errstate(all="ignore"):
        p, y = rescaled(pred, scale, shift), rescaled(real, scale, shift)
        assert p.dtype == np.float32 and y.dtype == np.float32 and p.ndim == 3 and p.shape == y.shape
        null = np.float32(null_val)
        m = ~np.isnan(y) if np.isnan(null) else ~(np.abs(y - null) <= np.float32(5e-5))
        d = p - y
        ad, sq = np.abs(d), d * d
        y0 = np.where(np.abs(y) < np.float32(1e-4), np.float32(0.0), y)
        m0 = ~(np.abs(y0) <= np.float32(5e-5))
        t = np.abs(np.abs(p - y0) / y0)
        assert ad.dtype == sq.dtype == t.dtype == np.float32

        def total(term, mask):          # a NaN term adds 0 and still counts
            return np.where(mask & ~np.isnan(term), term, np.float32(0.0)).astype(np.float64).sum(axis=0)
        return np.stack([total(ad, m), total(sq, m), m.astype(np.float64).sum(axis=0), total(t, m0), m0.astype(np.float64).sum(axis=0)])


def finished(table):
    """f64 [5, H, N] -> f64 [N, H + 1, 3]: MAE, RMSE, MAPE of every node per horizon, and in row H over all horizons (count 0 -> 0)"""
    table = np.asarray(table, dtype=np.float64)
    both = np.concatenate([table, table.sum(axis=1, keepdims=True)], axis=1)          # [5, H + 1, N]

    def ratio(s, c):
        return np.where(c > 0.0, s / np.where(c > 0.0, c, 1.0), 0.0)
    out = np.stack([ratio(both[0], both[2]), np.sqrt(ratio(both[1], both[2])), ratio(both[3], both[4])], axis=-1)          # [H + 1, N, 3]
    return np.ascontiguousarray(out.transpose(1, 0, 2))
