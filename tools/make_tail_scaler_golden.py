"""Reference side of the tests of the tails under a NaN ``null_val`` and under per-node scalers (tests/test_gpu_tail_scalers.py,
tests/test_tail_scaler_host.py): the reference's OWN step_loss, re_standard_transform and masked_mae / masked_rmse / masked_mape, loaded
the way tools/make_train_tail_golden.py loads them, on small hand-built cases -- rescale, slice [:, :k], loss, backward, three metrics as
the runner evaluates a training iteration (basicts/runners/base_tsf_runner.py:237-254), the per-horizon / overall / per-batch table of
its test and validation passes (the format of tools/make_eval_metrics_golden.py), and the pre-training tail on the masked tokens (as
tools/make_pretrain_tail_golden.py).  All in f32 on the CPU.  Needs the reference checkout (oracle/reference_loader.py).  Writes
tests/golden/tail_scaler_cases.npz.

    python tools/make_tail_scaler_golden.py

A per-node scaler is what ``standard_transform(..., norm_each_channel=True)`` pickles: float64 ``mean`` and ``std`` of shape [1, N, 1],
here with mean in [150, 250] and std in [20, 80] drawn per node, so that a swapped or flattened node index moves every result far
outside the tests' tolerances.  The scalar scaler is (mean 207.227, std 38.25).

Keys.  `shapes` (names), `ks`, `pairs` = (nan_scalar, zero_node, nan_node): (null_val, scaler) = (NaN, scalar), (0.0, per-node),
(NaN, per-node); `scalar.mean`, `scalar.std` f64.  Per shape s of (a, b, c, one): s.theta, s.prior f32 [B, 16, 16]; s.coef f32; s.dtheta
f32 [B, 16, 16] (it depends on neither k nor the pair); s.mean_n, s.std_n f64 [1, N, 1]; s.split (batch sizes of the validation
split); s.C; and the inputs in a form that stays small on disk -- s.raw f32 [B, 12, N], s.q int8 [B, 12, N], s.noise_step f32,
s.nan_labels int64 [., 3], s.nan_pred int64 [3] -- from which ``inputs(z, s, kind)`` below builds the normalised prediction [B, 12, N]
and the batch tensor [B, 12, N, C] with the label in channel 0 for either kind of scaler (the tests call the same function).  Per pair
p and k: s.p.k.loss f32, s.p.k.metrics f32 [3] (MAE, RMSE, MAPE), s.p.k.dpred f32 [B, 12, N] (w.r.t. the NORMALISED prediction; NaN
where the prediction or the label is NaN: the reference's gradient of a NaN term is NaN, the kernels' is defined as 0); per pair:
s.p.per_horizon f64 [12, 3], s.p.overall f64 [3], s.p.batch_mean_split f64 [3].  `allnan` is shape `a` whose labels of horizon 0 are
all NaN (pair nan_node only, results only): at k = 1 nothing counts and the result is the graph term alone with zero metrics.
Pre-training, per case c in `pretrain_cases` (pair nan_scalar only): c.r f32 [S, P, 12]; c.series f32 [S, P * 12]; c.mk int32 [Pm];
c.Pu, c.B, c.N int64; c.loss f32; c.metrics f32 [3]; c.dr f32 [S, P, 12] (NaN where r or the label is)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 5, 12)
H = 12
PAIRS = {"nan_scalar": (float("nan"), "scalar"), "zero_node": (0.0, "node"), "nan_node": (float("nan"), "node")}
SHAPES = {"a": (3, 5, 1), "b": (2, 70, 3), "c": (4, 307, 3), "one": (1, 1, 1)}          # (B, N, C)
SPLITS = {"a": [2, 1], "b": [1, 1], "c": [3, 1], "one": [1], "allnan": [2, 1]}
SCALAR_MEAN, SCALAR_STD = 207.227, 38.25
PRETRAIN = {"p18": (2, 9, 16, 12), "p5": (1, 5, 8, 6)}          # (B, N, P, Pm): S = B * N
PATH = os.path.join(ROOT, "tests", "golden", "tail_scaler_cases.npz")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def reference_functions():
    """-> (step_loss, re_standard_transform, [masked_mae, masked_rmse, masked_mape]) of the reference"""
    return _tool("make_train_tail_golden").reference_functions()


def node_scaler(rng, N):
    return rng.uniform(150.0, 250.0, size=(1, N, 1)), rng.uniform(20.0, 80.0, size=(1, N, 1))


def raw_case(rng, B, N, noise):
    """the raw side of labels_and_pred of tools/make_train_tail_golden.py, kept small on disk: a raw series of whole numbers (f32) in which a
    fifth of the values are exactly 0 and two dozen (as many as fit) sit next to the 5e-5 / 1e-4 thresholds, the prediction's noise as
    non-zero int8 multiples of noise / 32, a handful of NaN labels and one NaN prediction on a counted label of horizon 0.  Shape `one` (12
    labels): one zero, one threshold value, no NaN label, the NaN prediction at horizon 3 (horizon 0 must say something at k = 1)"""
    raw = np.rint(rng.uniform(20.0, 600.0, size=(B, H, N))).astype(np.float32)
    q = np.clip(np.rint(rng.normal(0.0, 32.0, size=raw.shape)), -127, 127).astype(np.int8)
    q[q == 0] = 1          # no prediction equals its label: every counted element has a gradient
    if raw.size > 24:
        raw[rng.random(raw.shape) < 0.2] = 0.0
        near = rng.permutation(raw.size)[:24]
        raw.reshape(-1)[near] = np.repeat(np.float32([2e-5, 4e-5, 5e-5, 6e-5, 9e-5, 1.2e-4]), 4)
        nan_labels = np.stack(np.unravel_index(rng.permutation(raw.size)[:5], raw.shape), axis=1).astype(np.int64)
        h_nan = 0
    else:
        raw[0, 5, 0], raw[0, 7, 0] = 0.0, 6e-5
        nan_labels = np.zeros((0, 3), dtype=np.int64)
        h_nan = 3
    ok = raw[:, h_nan, :] > 1.0
    ok[nan_labels[nan_labels[:, 1] == h_nan][:, 0], nan_labels[nan_labels[:, 1] == h_nan][:, 2]] = False
    b, n = np.argwhere(ok)[0]          # a counted label under every pair
    return dict(raw=raw, q=q, noise_step=np.float32(noise / 32.0), nan_labels=nan_labels, nan_pred=np.array([b, h_nan, n], dtype=np.int64))


def inputs(z, name, kind):
    """-> (pred f32 [B, 12, N], real f32 [B, 12, N, C]) of shape `name` under the scaler `kind` ("scalar" / "node") from the fixture's
    (or compute()'s) arrays: the label, channel 0, is the normalised image (raw - mean) / std of the raw series, the prediction is the
    label plus the noise in normalised units, channel c > 0 holds the small integer c + 1 -- in float32 operations that round the same
    everywhere.  `allnan` is shape `a` with the labels of horizon 0 all NaN"""
    src = "a" if name == "allnan" else name
    raw = z[f"{src}.raw"]
    B, _, N = raw.shape
    if kind == "scalar":
        mean_n, std_n = np.full(N, z["scalar.mean"], dtype=np.float32), np.full(N, z["scalar.std"], dtype=np.float32)
    else:
        mean_n, std_n = z[f"{src}.mean_n"].reshape(N).astype(np.float32), z[f"{src}.std_n"].reshape(N).astype(np.float32)
    y = ((raw - mean_n) / std_n).astype(np.float32)
    pred = (y + (z[f"{src}.q"].astype(np.float32) * np.float32(z[f"{src}.noise_step"])) / std_n).astype(np.float32)
    real = np.empty(raw.shape + (int(z[f"{src}.C"]),), dtype=np.float32)
    real[...] = np.arange(1, real.shape[-1] + 1, dtype=np.float32)
    real[..., 0] = y
    for b, h, n in z[f"{src}.nan_labels"]:
        real[b, h, n, 0] = np.nan
    b, h, n = z[f"{src}.nan_pred"]
    pred[b, h, n] = np.nan
    if name == "allnan":
        real[:, 0, :, 0] = np.nan
    return pred, real


def graph(rng, B):
    theta = np.clip(rng.random((B, 16, 16)), 1e-4, 1 - 1e-4).astype(np.float32)
    prior = (rng.random((B, 16, 16)) < 0.1).astype(np.float32)
    return theta, prior


def build_cases():
    """-> the fixture's inputs: per shape s the keys s.raw, s.q, s.noise_step, s.nan_labels, s.nan_pred, s.C, s.theta, s.prior, s.coef,
    s.mean_n, s.std_n, s.split; scalar.mean, scalar.std"""
    rng = np.random.default_rng(20241020)
    out = {"scalar.mean": np.float64(SCALAR_MEAN), "scalar.std": np.float64(SCALAR_STD)}
    for (name, (B, N, C)), coef, noise in zip(SHAPES.items(), (1.0, 0.5, 0.25, 1.0), (4.0, 8.0, 20.0, 4.0)):
        case = raw_case(rng, B, N, noise)
        case["theta"], case["prior"] = graph(rng, B)
        case["mean_n"], case["std_n"] = node_scaler(rng, N)
        case.update(coef=np.float32(coef), C=np.int64(C), split=np.array(SPLITS[name], dtype=np.int64))
        out.update({f"{name}.{key}": v for key, v in case.items()})
    return out


def case_of(z, name):
    """what the recording functions take: the graph, the node scaler and both kinds of inputs of shape `name`"""
    src = "a" if name == "allnan" else name
    case = {key: z[f"{src}.{key}"] for key in ("theta", "prior", "coef", "mean_n", "std_n")}
    for kind in ("scalar", "node"):
        case[kind] = inputs(z, name, kind)
    return case


def pairs_of(name):
    return ("nan_node",) if name == "allnan" else tuple(PAIRS)


def scaler_of(case, kind):
    return (SCALAR_MEAN, SCALAR_STD) if kind == "scalar" else (case["mean_n"], case["std_n"])


def counted(y, null_val):
    """the labels the reference's masked_mae counts (mae.py:17-21) on the rescaled labels y"""
    return ~torch.isnan(y) if null_val != null_val else ~torch.isclose(y, torch.full_like(y, null_val), atol=5e-5, rtol=0.0)


def record_tail(fns, case, pair):
    step_loss, rescale, metrics = fns
    null_val, kind = PAIRS[pair]
    mean, std = scaler_of(case, kind)
    pred0, real0 = case[kind]
    real = torch.from_numpy(real0[..., :1])
    out = {}
    for k in KS:
        pred = torch.from_numpy(pred0)[..., None].clone().requires_grad_(True)
        theta = torch.from_numpy(case["theta"]).clone().requires_grad_(True)
        p = rescale(pred, mean=mean, std=std)[:, :k, :, :]
        y = rescale(real, mean=mean, std=std)[:, :k, :, :]
        loss = step_loss(p, y, theta, torch.from_numpy(case["prior"]), float(case["coef"]), null_val=null_val)
        dpred, dtheta = torch.autograd.grad(loss, [pred, theta])
        out[f"{pair}.{k}.loss"] = np.float32(loss.item())
        out[f"{pair}.{k}.metrics"] = np.array([f(p.detach(), y, null_val=null_val).item() for f in metrics], dtype=np.float32)
        out[f"{pair}.{k}.dpred"] = dpred[..., 0].numpy().copy()
        out[f"{pair}.{k}.share"] = float(counted(y, null_val).float().mean())
        out["dtheta"] = dtheta.numpy().copy()
    return out


def record_table(fns, case, pair, split):
    """tools/make_eval_metrics_golden.py's table: per horizon, over everything, and the mean over a split into batches"""
    _, rescale, metrics = fns
    null_val, kind = PAIRS[pair]
    mean, std = scaler_of(case, kind)
    pred0, real0 = case[kind]
    p = rescale(torch.from_numpy(pred0)[..., None], mean=mean, std=std)
    y = rescale(torch.from_numpy(real0[..., :1]), mean=mean, std=std)

    def three(a, b):
        return [float(f(a, b, null_val=null_val).item()) for f in metrics]
    per_h = np.array([three(p[:, h], y[:, h]) for h in range(H)], dtype=np.float64)
    at, rows = 0, []
    for n in split:
        rows.append(three(p[at:at + n], y[at:at + n]))
        at += n
    assert at == p.shape[0]
    return {f"{pair}.per_horizon": per_h, f"{pair}.overall": np.array(three(p, y), dtype=np.float64),
            f"{pair}.batch_mean_split": np.mean(np.array(rows, dtype=np.float64), axis=0)}


def build_pretrain_cases():
    """the cases of tools/make_pretrain_tail_golden.py's kind at two more shapes, under the scalar scaler, with a handful of NaN labels and
    one NaN reconstruction on a counted label"""
    pt = _tool("make_pretrain_tail_golden")
    rng = np.random.default_rng(20241021)
    cases = {}
    for name, (B, N, P, Pm) in PRETRAIN.items():
        mk = sorted(rng.permutation(P)[:Pm].tolist())
        r, series = pt.tensors(rng, B * N, P, mk, SCALAR_STD, SCALAR_MEAN, 8.0)
        lab = series.reshape(B * N, P, 12)
        for i in rng.permutation(B * N * Pm * 12)[:5]:
            s, j, e = np.unravel_index(i, (B * N, Pm, 12))
            lab[s, mk[j], e] = np.nan
        back = lab[:, mk, :] * np.float32(SCALAR_STD) + np.float32(SCALAR_MEAN)
        s, j, e = np.argwhere(np.abs(back) > 1.0)[3]
        r[s, P - Pm + j, e] = np.nan
        cases[name] = dict(r=r, series=series, mk=np.array(mk, dtype=np.int32), Pu=P - Pm, B=B, N=N)
    return pt, cases


def record_pretrain(fns, pt, case):
    _, rescale, metrics = fns
    r = torch.from_numpy(case["r"]).clone().requires_grad_(True)
    recon, label = pt.select(case, r, torch.from_numpy(case["series"]))
    p, y = rescale(recon, mean=SCALAR_MEAN, std=SCALAR_STD), rescale(label, mean=SCALAR_MEAN, std=SCALAR_STD)
    nan = float("nan")
    loss = metrics[0](p, y, null_val=nan)
    dr, = torch.autograd.grad(loss, [r])
    share = float((~torch.isnan(y)).float().mean())
    return {"loss": np.float32(loss.item()), "metrics": np.array([f(p.detach(), y, null_val=nan).item() for f in metrics], dtype=np.float32),
            "dr": dr.numpy().copy()}, share


def compute():
    """-> the fixture's content as a dict of numpy arrays"""
    fns = reference_functions()
    out = build_cases()
    out.update({"shapes": np.array(list(SHAPES) + ["allnan"]), "ks": np.array(KS, dtype=np.int64), "pairs": np.array(list(PAIRS))})
    for name in out["shapes"]:
        case = case_of(out, name)
        for pair in pairs_of(name):
            kind = PAIRS[pair][1]
            nan_at = np.isnan(case[kind][0]) | np.isnan(case[kind][1][..., 0])
            for key, v in record_tail(fns, case, pair).items():
                if key.endswith(".share"):
                    # a test that quietly runs on nothing is worthless: the reference counts at least half of the labels of every slice
                    k = int(key.split(".")[1])
                    assert (v == 0.0 if (name, k) == ("allnan", 1) else v >= 0.5), (name, key, v)
                    continue
                finite = np.isfinite(v) | nan_at if key.endswith(".dpred") else np.isfinite(v)
                assert finite.all(), (name, key)
                if key == "dtheta":
                    src = "a" if name == "allnan" else name
                    assert f"{src}.dtheta" not in out or np.array_equal(out[f"{src}.dtheta"], v), name
                    out[f"{src}.dtheta"] = v
                    continue
                if key.endswith(".metrics") and (name, key) != ("allnan", "nan_node.1.metrics"):
                    assert (v > 0).all(), (name, key, v)
                out[f"{name}.{key}"] = v
            for key, v in record_table(fns, case, pair, SPLITS[name]).items():
                assert np.isfinite(v).all(), (name, key)
                out[f"{name}.{key}"] = v
    assert (out["allnan.nan_node.1.metrics"] == 0).all() and (out["allnan.nan_node.per_horizon"][0] == 0).all()
    pt, pcases = build_pretrain_cases()
    out["pretrain_cases"] = np.array(list(pcases))
    for name, case in pcases.items():
        for key in ("r", "series", "mk"):
            out[f"{name}.{key}"] = case[key]
        for key in ("Pu", "B", "N"):
            out[f"{name}.{key}"] = np.int64(case[key])
        rec, share = record_pretrain(fns, pt, case)
        assert share >= 0.5, (name, share)
        _, label = pt.select(case, torch.from_numpy(case["r"]), torch.from_numpy(case["series"]))
        for key, v in rec.items():
            if key == "dr":
                S, P = case["r"].shape[:2]
                lab_nan = np.zeros((S, P, 12), dtype=bool)
                lab_nan[:, case["Pu"]:, :] = np.isnan(case["series"].reshape(S, P, 12)[:, case["mk"], :])
                assert (np.isfinite(v) | np.isnan(case["r"]) | lab_nan).all(), (name, key)
            else:
                assert np.isfinite(v).all(), (name, key)
            out[f"{name}.{key}"] = v
    return out


def main():
    out = compute()
    for name in out["shapes"]:
        for pair in pairs_of(name):
            print(name, pair, {k: (float(out[f"{name}.{pair}.{k}.loss"]), out[f"{name}.{pair}.{k}.metrics"].tolist()) for k in KS})
    for name in out["pretrain_cases"]:
        print(name, out[f"{name}.r"].shape, float(out[f"{name}.loss"]), out[f"{name}.metrics"].tolist())
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
