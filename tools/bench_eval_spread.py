"""What window-keyed eval noise and the native test pass cost on ONE rank, through the runner's own hooks: config C2 (PEMS04 shape:
N = 307, L = 4032, B = 8, T = 16 992, random-init weights, bf16 mode, f16 encoder operands), `--batches` loader batches of origins from
a ``DeviceForecastingDataset`` behind a ``DataLoader`` (no workers), in one process, the legs alternated `--repeats` times after a
warm-up of every leg; medians and the run-to-run range per leg:

    val_position        one validation pass, ``native_eval=True``: the graph learner's noise keyed by the position in the batch (today's)
    val_window          the same pass with ``eval_noise="window"``: keyed by the forecast origin (``step_dgl_edges_forward_keyed``)
    test_base           the base class's forecasting ``test()`` (basicts/runners/base_tsf_runner.py:277-318, restated below): every
                        prediction kept, concatenated, rescaled, sliced per horizon, 39 ``.item()``
    test_native         ``native_test=True``: one ``EvalMetrics`` launch per batch, one read-back

The harness of tools/bench_runner_eval.py: a pass is timed with a host clock that ends in one device synchronise and starts without a
kept g.  ``host_readbacks_per_pass`` counts ``.item()`` / ``.cpu()`` / ``.tolist()`` on device tensors in one extra, untimed pass.

A pass spread over several GPUs (``spread_eval=True``) CANNOT be timed on one card -- two ranks on one device share it -- and is not:
``batches_per_rank`` lists what ``eval_rank_chunks`` gives each rank of 2 and of 8 for this pass, which is all that is claimed.

    python tools/bench_eval_spread.py --out profiles/eval_spread.json
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from bench_runner_eval import BaseRunner, ReadbackCounter  # noqa: E402


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line)


class TestRunner(BaseRunner):
    """``BaseRunner`` plus the forecasting ``test()`` of base_tsf_runner.py:277-318, restated"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.evaluation_horizons = range(12)
        self.logger = _Log()
        self.test_data_loader = None

    def build_test_data_loader(self, cfg):
        return torch.utils.data.DataLoader(cfg["val_dataset"], batch_size=cfg["batch_size"], shuffle=False)

    @torch.no_grad()
    def test(self):
        prediction, real_value = [], []
        for _, data in enumerate(self.test_data_loader):
            forward_return = self.forward(data, epoch=None, iter_num=None, train=False)
            prediction.append(forward_return[0])
            real_value.append(forward_return[1])
        prediction, real_value = torch.cat(prediction, dim=0), torch.cat(real_value, dim=0)
        mean, std = self.scaler["args"]["mean"], self.scaler["args"]["std"]
        prediction, real_value = prediction * std + mean, real_value * std + mean
        for i in self.evaluation_horizons:
            metric_repr = ""
            for metric_name, metric_func in self.metrics.items():
                metric_item = self.metric_forward(metric_func, [prediction[:, i, :, :], real_value[:, i, :, :]])
                metric_repr += ", Test {0}: {1:.4f}".format(metric_name, metric_item.item())
            self.logger.info(("Evaluate best model on test data for horizon {:d}" + metric_repr).format(i + 1))
        for metric_name, metric_func in self.metrics.items():
            self.update_epoch_meter("test_" + metric_name, self.metric_forward(metric_func, [prediction, real_value]).item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="STEP_PEMS04")
    ap.add_argument("--batches", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from step_amd.evaluate import eval_rank_chunks
    from step_amd.runner import DeviceForecastingDataset, native_runner
    cfg = bench.CONFIGS[args.config]
    N, L, B = cfg["N"], cfg["L"], cfg["B"]
    series = bench.synth_series(cfg["T_all"], N)
    model = bench.make_model(cfg, series).cuda()
    model.matmul_precision = "bf16"
    model.tsformer.encoder_operand = "f16"
    model.eval()
    first = cfg["T_train"]
    windows = args.batches * B
    assert first + windows + 12 <= cfg["T_all"]
    with tempfile.TemporaryDirectory() as tmp:
        index = [(t - 12, t, t + 12) for t in range(first, first + windows)]
        with open(os.path.join(tmp, "data.pkl"), "wb") as f:
            pickle.dump({"processed_data": series}, f)
        with open(os.path.join(tmp, "index.pkl"), "wb") as f:
            pickle.dump({"train": index[:1], "valid": index, "test": index}, f)
        dataset = DeviceForecastingDataset(os.path.join(tmp, "data.pkl"), os.path.join(tmp, "index.pkl"), "valid", L)
    switches = {"val_position": {"native_eval": True}, "val_window": {"native_eval": True, "eval_noise": "window"},
                "test_base": {}, "test_native": {"native_test": True}}
    noise = {"val_position": "position", "val_window": "window", "test_base": "position", "test_native": "position"}
    run_cfg = {"model": model, "scaler": (207.2, 38.4), "val_dataset": dataset, "batch_size": B}          # any finite scaler
    runners = {}
    for name, kw in switches.items():
        r = runners[name] = native_runner(TestRunner, **kw)(run_cfg)
        r.val_data_loader, r.test_data_loader = r.build_val_data_loader(run_cfg), r.build_test_data_loader(run_cfg)

    def one_pass(name):
        runner = runners[name]
        model.eval_noise = noise[name]          # (build_*_data_loader set it for whoever was built last)
        model._drop_eval_g()
        runner.meters = {}
        del runner.logger.lines[:]
        torch.cuda.synchronize()
        t = time.perf_counter()
        if name.startswith("val_"):
            with torch.no_grad():
                for i, data in enumerate(runner.val_data_loader):
                    runner.val_iters(i, data)
            runner.flush_meters()
        else:
            runner.test()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert len(runner.meters) == 3 and (name.startswith("val_") or len(runner.logger.lines) == 12), (runner.meters, runner.logger.lines)
        return dt, {k: s / c for k, (s, c) in runner.meters.items()}

    for name in switches:          # warm-up of every leg, past the launches the float16 range guard checks at once
        one_pass(name)
        one_pass(name)
    times, meters = {name: [] for name in switches}, {}
    for _ in range(args.repeats):
        for name in switches:
            dt, meters[name] = one_pass(name)
            times[name].append(dt)
    readbacks = {}
    for name in switches:
        with ReadbackCounter() as counter:
            one_pass(name)
        readbacks[name] = counter.count
    out = {"tool": "bench_eval_spread", "config": args.config, "N": N, "L": L, "B": B, "batches": args.batches, "windows": windows,
           "repeats": args.repeats, "matmul_precision": "bf16", "encoder_operand": model.tsformer.encoder_operand_in_use,
           "device": torch.cuda.get_device_name(0), "legs": {},
           "batches_per_rank": {str(w): [len(eval_rank_chunks(args.batches, r, w)) for r in range(w)] for w in (2, 8)},
           "spread_pass_timed": False}
    for name, ts in times.items():
        ms = sorted(1e3 * t for t in ts)
        med = ms[len(ms) // 2]
        out["legs"][name] = {"ms_per_pass": med, "ms_per_pass_runs": [1e3 * t for t in ts], "range_ms": [ms[0], ms[-1]],
                             "ms_per_loader_batch": med / args.batches, "host_readbacks_per_pass": readbacks[name], "meters": meters[name]}
    for a, b in (("val_window", "val_position"), ("test_native", "test_base")):
        la, lb = out["legs"][a], out["legs"][b]
        la["minus_" + b + "_ms"] = la["ms_per_pass"] - lb["ms_per_pass"]
        la["ranges_overlap"] = la["range_ms"][0] <= lb["range_ms"][1] and lb["range_ms"][0] <= la["range_ms"][1]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
