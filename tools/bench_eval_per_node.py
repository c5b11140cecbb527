"""What the per-node evaluation table and the export of the predictions in data units cost, on ONE card.

Kernel alone: ``step_eval_node_metrics_accumulate`` (csrc/eval_nodes.hip) between two device events on an idle device, median of
``--iters`` launches after a warm-up, at (B, N) = (8, 307), (64, 307), (8, 883) with H = 12 -- the prediction [B, H, N, 1], the label
channel 0 of [B, H, N, 3], as the evaluation pass hands them over -- without and with ``out``, next to
``step_eval_metrics_accumulate`` at the same shapes (the launch it is issued beside).

Whole pass: config C2 (PEMS04 shape: N = 307, L = 4032, B = 8, random-init weights, bf16 mode, f16 encoder operands), ``--batches``
batches through ``STEP.evaluate`` on a ``DeviceWindowLoader``, four legs alternated ``--repeats`` times after a warm-up of every leg,
medians and run-to-run ranges: ``plain`` (today's pass), ``per_node`` (``per_node=True``), ``predictions_normalised``
(``return_predictions=True``: a ``copy_`` per batch) and ``predictions_data`` (``return_predictions="data"``: stored by the kernel).
A pass is timed with a host clock that ends in one device synchronise.

    python tools/bench_eval_per_node.py --out profiles/eval_per_node.json

``--default-lines FILE``: a JSON file of bench.py headline lines recorded in the same session ({"command": .., "parent": [..],
"tree": [..]}, whole result lines) is folded into the record as ``default_training_step`` with the ranges' overlap."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

H = 12
SHAPES = [(8, 307), (64, 307), (8, 883)]


def median_range(xs):
    s = sorted(xs)
    return s[len(s) // 2], [s[0], s[-1]]


def kernel_alone(iters, warmup):
    from step_amd import _lib
    rows = []
    gen = torch.Generator().manual_seed(0)
    for B, N in SHAPES:
        pred = torch.randn(B, H, N, 1, generator=gen).cuda()
        real = torch.randn(B, H, N, 3, generator=gen).cuda()
        real[..., 0][torch.rand(B, H, N, generator=gen).cuda() < 0.1] = -207.2 / 38.4          # a tenth of the labels rescale to 0
        acc = torch.zeros(_lib.lib().step_eval_metrics_acc_doubles(H), dtype=torch.float64, device="cuda")
        table = torch.zeros(_lib.lib().step_eval_node_table_doubles(H, N), dtype=torch.float64, device="cuda")
        out = torch.empty(B, H, N, device="cuda")
        views = [_lib.ptr(pred), H * N, N, 1, ctypes.c_void_p(real.data_ptr()), 3 * H * N, 3 * N, 3, B, H, N, 38.4, 207.2, 0.0]
        legs = {"eval_metrics_accumulate": lambda: _lib.call("step_eval_metrics_accumulate", *views, _lib.ptr(acc), _lib.stream()),
                "eval_node_metrics_accumulate": lambda: _lib.call("step_eval_node_metrics_accumulate", *views, _lib.ptr(table), None, _lib.stream()),
                "eval_node_metrics_accumulate_out": lambda: _lib.call("step_eval_node_metrics_accumulate", *views, _lib.ptr(table),
                                                                      _lib.ptr(out), _lib.stream())}
        row = {"B": B, "H": H, "N": N}
        for name, launch in legs.items():
            for _ in range(warmup):
                launch()
            torch.cuda.synchronize()
            us = []
            for _ in range(iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()          # idle device: the next launch starts behind an empty queue
                us.append(1e3 * a.elapsed_time(b))
            med, rng = median_range(us)
            s = sorted(us)
            row[name] = {"device_us": med, "device_us_p10_p90": [s[len(s) // 10], s[(9 * len(s)) // 10]], "device_us_range": rng}
        rows.append(row)
    return rows


def whole_pass(config, batches, repeats):
    from step_amd import DeviceWindowLoader
    cfg = bench.CONFIGS[config]
    N, L, B = cfg["N"], cfg["L"], cfg["B"]
    series = bench.synth_series(cfg["T_all"], N)
    model = bench.make_model(cfg, series).cuda()
    model.matmul_precision = "bf16"
    model.tsformer.encoder_operand = "f16"
    model.eval()
    loader = DeviceWindowLoader(torch.from_numpy(series).cuda(), L)
    first = cfg["T_train"]
    origins = list(range(first, first + batches * B))
    assert origins[-1] + 12 <= cfg["T_all"]
    legs = {"plain": {}, "per_node": {"per_node": True}, "predictions_normalised": {"return_predictions": True},
            "predictions_data": {"return_predictions": "data"}}

    def one_pass(name):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = model.evaluate(loader, origins, scaler=(207.2, 38.4), null_val=0.0, batch_size=B, **legs[name])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        res = res[0] if isinstance(res, tuple) else res
        return dt, res
    for name in legs:          # warm-up of every leg, past the launches the float16 range guard checks at once
        one_pass(name)
        one_pass(name)
    times, last = {name: [] for name in legs}, {}
    for _ in range(repeats):
        for name in legs:
            dt, last[name] = one_pass(name)
            times[name].append(dt)
    out = {"config": config, "N": N, "L": L, "B": B, "batches": batches, "windows": len(origins), "repeats": repeats,
           "matmul_precision": "bf16", "encoder_operand": model.tsformer.encoder_operand_in_use, "legs": {}}
    for name, ts in times.items():
        med, rng = median_range([1e3 * t for t in ts])
        out["legs"][name] = {"ms_per_pass": med, "ms_per_pass_runs": [1e3 * t for t in ts], "range_ms": rng, "ms_per_batch": med / batches,
                             "overall": last[name].overall.tolist()}
    for a, b in (("per_node", "plain"), ("predictions_data", "predictions_normalised"), ("predictions_data", "plain")):
        la, lb = out["legs"][a], out["legs"][b]
        la["minus_" + b + "_us_per_batch"] = 1e3 * (la["ms_per_pass"] - lb["ms_per_pass"]) / batches
        la["ranges_overlap_" + b] = la["range_ms"][0] <= lb["range_ms"][1] and lb["range_ms"][0] <= la["range_ms"][1]
    worst = last["per_node"].per_node_overall[:, 0]
    out["per_node_overall_mae_min_max"] = [float(worst.min()), float(worst.max())]
    return out


def default_lines(path):
    with open(path) as f:
        rec = json.load(f)
    out = {"command": rec["command"], "what": rec.get("what", ""), "unit": None, "runs": {}, "ranges": {}}
    for side in ("parent", "tree"):
        lines = rec[side]
        out["unit"] = lines[0].get("unit", out["unit"])
        out["runs"][side] = [ln["value"] for ln in lines]
        out["ranges"][side] = [min(out["runs"][side]), max(out["runs"][side])]
    (a0, a1), (b0, b1) = out["ranges"]["parent"], out["ranges"]["tree"]
    out["ranges_overlap"] = a0 <= b1 and b0 <= a1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="STEP_PEMS04")
    ap.add_argument("--batches", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--default-lines", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = {"tool": "bench_eval_per_node", "device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
           "kernel_alone": kernel_alone(args.iters, args.warmup), "whole_pass": whole_pass(args.config, args.batches, args.repeats)}
    if args.default_lines:
        out["default_training_step"] = default_lines(args.default_lines)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
