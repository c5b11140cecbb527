"""What STEP.eval_cache_bytes and STEP.evaluate are worth on a validation pass: config C2 (PEMS04 shape: N = 307, L = 4032, B = 8,
T = 13 599, random-init weights, bf16 mode, f16 encoder operands), 250 sequential batches of validation origins through
DeviceWindowLoader, in one process, alternated `--repeats` times after a warm-up of every shape:

    off / on_first / on_later                     the forward loop written by hand (no metrics): cache off; cache on, first pass
                                                  (computes and stores); cache on, later pass (loads)
    evaluate_off / evaluate_on_later              STEP.evaluate over the same windows at the config's batch size: the same forwards
                                                  plus the per-horizon metrics on the device and their one read-back
    evaluate_off_b<E> / evaluate_on_later_b<E>    the same at `--eval-batch` E windows per forward (default 64)

A pass is timed with a host clock that ends in one device synchronise.  Every cached pass starts without a kept g, as after the
training epoch that precedes a real validation pass.  `ms_per_batch` is per `B` windows in every leg, whatever the forward's batch.

    python tools/bench_eval_pass.py --out profiles/eval_pass_C2.json

Not measured here: the larger configs (C4 / C5) and anything through the reference's runner."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="STEP_PEMS04")
    ap.add_argument("--batches", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget-mib", type=int, default=1024)
    ap.add_argument("--eval-batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from step_amd import DeviceWindowLoader
    cfg = bench.CONFIGS[args.config]
    N, L, B = cfg["N"], cfg["L"], cfg["B"]
    series = bench.synth_series(cfg["T_all"], N)
    model = bench.make_model(cfg, series).cuda()
    model.matmul_precision = "bf16"
    model.tsformer.encoder_operand = "f16"
    model.eval()
    loader = DeviceWindowLoader(torch.from_numpy(series).cuda(), L)
    first = cfg["T_train"]                                        # validation origins follow the training split, in order (SHUFFLE = False)
    assert first + args.batches * B + 12 <= cfg["T_all"]
    batches = [torch.arange(first + i * B, first + (i + 1) * B, dtype=torch.int64) for i in range(args.batches)]

    def one_pass(which):
        torch.cuda.synchronize()
        t = time.perf_counter()
        with torch.no_grad():
            for t0 in which:
                hist, ref, _fut = loader.batch(t0)
                model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=0, epoch=1)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    origins = [int(t) for t0 in batches for t in t0]
    E = args.eval_batch
    scaler = (207.2, 38.4)          # any finite scaler: the metric kernel's work does not depend on it
    tables = {}

    def evaluate_pass(which, batch):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = model.evaluate(loader, which, scaler=scaler, null_val=0.0, batch_size=batch)          # ends in its one read-back
        torch.cuda.synchronize()
        tables[batch] = res
        return time.perf_counter() - t

    def leg(name):
        if name == "off" or name.startswith("evaluate_off"):
            model.eval_cache_bytes = 0
        else:
            model.eval_cache_bytes = args.budget_mib << 20
            model._drop_eval_g()
            if name == "on_first":
                model.clear_eval_cache()
        if name.startswith("evaluate"):
            return evaluate_pass(origins, E if name.endswith(f"_b{E}") else B)
        return one_pass(batches)

    # warm-up of every shape: the uncached forward (also past the launches the float16 range guard checks at once), a store, a load,
    # and the same through evaluate at both batch sizes
    one_pass(batches[:4])
    evaluate_pass(origins[:2 * E], B)
    evaluate_pass(origins[:2 * E], E)
    model.eval_cache_bytes = args.budget_mib << 20
    one_pass(batches[:4])
    one_pass(batches[:4])
    evaluate_pass(origins[:2 * E], E)
    evaluate_pass(origins[:2 * E], E)
    model.clear_eval_cache()
    names = ("off", "evaluate_off", f"evaluate_off_b{E}", "on_first", "on_later", "evaluate_on_later", f"evaluate_on_later_b{E}")
    times = {name: [] for name in names}
    held = 0
    for _ in range(args.repeats):
        for name in names:          # on_first refills the cache that the three later-pass legs behind it read
            times[name].append(leg(name))
        held = model._eval_cache.bytes_held
    windows = args.batches * B
    out = {"tool": "bench_eval_pass", "config": args.config, "N": N, "L": L, "B": B, "batches": args.batches, "repeats": args.repeats,
           "matmul_precision": "bf16", "encoder_operand": model.tsformer.encoder_operand_in_use, "device": torch.cuda.get_device_name(0),
           "eval_batch": E, "cache_bytes_held": int(held), "cache_budget_bytes": args.budget_mib << 20, "stats": dict(model.eval_cache_stats),
           "legs": {}}
    for name, ts in times.items():
        ms = [1e3 * t / args.batches for t in ts]
        out["legs"][name] = {"ms_per_batch": sorted(ms)[len(ms) // 2], "ms_per_batch_runs": ms, "spread_ms": max(ms) - min(ms),
                             "windows_per_s": windows / sorted(ts)[len(ts) // 2]}
    off, later, firstp = (out["legs"][k] for k in ("off", "on_later", "on_first"))
    out["later_pass_gain_ms"] = off["ms_per_batch"] - later["ms_per_batch"]
    out["first_pass_overhead_ms"] = firstp["ms_per_batch"] - off["ms_per_batch"]
    out["largest_spread_ms"] = max(v["spread_ms"] for v in out["legs"].values())
    # evaluate against the hand-written loop of the same cache state, per B windows (negative: evaluate is faster)
    ms = {k: v["ms_per_batch"] for k, v in out["legs"].items()}
    out["evaluate_minus_loop_ms"] = {"off": ms["evaluate_off"] - ms["off"], "on_later": ms["evaluate_on_later"] - ms["on_later"],
                                     f"off_b{E}": ms[f"evaluate_off_b{E}"] - ms["off"],
                                     f"on_later_b{E}": ms[f"evaluate_on_later_b{E}"] - ms["on_later"]}
    out["evaluate_overall"] = {f"b{b}": dict(zip(("MAE", "RMSE", "MAPE"), (float(x) for x in r.overall))) for b, r in sorted(tables.items())}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
