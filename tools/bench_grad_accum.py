"""Gradient accumulation (``set_grad_accumulation(k)`` + ``FusedAdamClip``) timed against k separate optimizer steps of the k = 1 loop, in
one session (needs a GPU; synthetic series, nothing of the reference):

  (a) separate   k times  zero_grad -> forward -> backward -> step        (k = 1: today's loop; k micro-batches cost k of everything)
  (b) group      zero_grad -> k x (forward -> (loss / k).backward()) -> step      (the graph learner's global forward and backward, the
                 87 MB fc weight gradient and the optimizer pass once per group)

at bench.py's configs C2 (STEP_PEMS04), C4 (STEP_PEMS07), C5 (SYNTH_4096) and C3 (TSFormer_PEMS-BAY pre-training) for k in {1, 2, 4}.
Both loops process the same k micro-batches per round and alternate inside one loop; a round is timed on the host (perf_counter
around it, the device idle before and after) and on the device (two events).  Reported: medians with p10 / p90 over --rounds rounds
after --warmup, per optimizer step and per micro-batch.  No look-ahead prefetch of the frozen branch here (bench.py's policy stays in
bench.py): the encoder runs inside every forward, so at C2 the figures are those of the unprefetched step.  There is no threshold.

    python tools/bench_grad_accum.py [--configs C2,C4,C5,C3] [--ks 1,2,4] [--out profiles/grad_accum.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                  # noqa: E402  (the config table, the synthetic series, the model builder)

NAMES = {"C2": "STEP_PEMS04", "C4": "STEP_PEMS07", "C5": "SYNTH_4096", "C3": "TSFormer_PEMS-BAY"}
MEAN, STD = 200.0, 150.0


def step_problem(cfg, matmul, nb):
    """-> (model, optimizer, micro(i): loss of resident micro-batch i)"""
    from step_amd import DeviceWindowLoader
    from step_amd.optim import FusedAdamClip
    from step_amd.step_loss import train_tail
    data = bench.synth_series(cfg["T_all"], cfg["N"])
    model = bench.make_model(cfg, data).cuda()
    model.train()
    model.matmul_precision = matmul
    opt = FusedAdamClip(model, lr=2e-3, weight_decay=1e-5, eps=1e-8, max_norm=3.0, param_grads=False)
    loader = DeviceWindowLoader(torch.from_numpy(data).cuda(), cfg["L"])
    rng = np.random.default_rng(7)
    batches = [loader.batch(rng.integers(cfg["L"], cfg["T_train"] - 12, size=cfg["B"])) for _ in range(nb)]

    def micro(i):
        hist, long_hist, fut = batches[i % nb]
        pred, theta, prior, coef = model(history_data=hist[..., :2], long_history_data=long_hist, future_data=None, batch_seen=i, epoch=1)
        return train_tail(pred, fut[..., :1], theta, prior, coef, null_val=0.0, rescale=(MEAN, STD), horizons=12)[0]
    return model, opt, micro


def pretrain_problem(cfg, matmul, nb):
    from step_amd import TSFormer
    from step_amd.optim import FusedAdamClip
    from step_amd.step_loss import masked_mae_native
    data = bench.synth_series(cfg["T_all"], cfg["N"])
    torch.manual_seed(0)
    random.seed(0)
    model = TSFormer(**bench.tsformer_args(cfg["L"], "pre-train")).cuda()
    model.train()
    model.matmul_precision = matmul
    model.flatten_parameters()
    opt = FusedAdamClip(model, lr=1e-3, weight_decay=0.0, eps=1e-8, betas=(0.9, 0.95), max_norm=5.0)
    dser = torch.from_numpy(data[:, :, :1]).cuda()
    rng = np.random.default_rng(99)
    batches = [torch.stack([dser[t - cfg["L"]:t] for t in rng.integers(cfg["L"], cfg["T_all"] - 12, size=cfg["B"])]) for _ in range(nb)]

    def micro(i):
        recon, label = model(history_data=batches[i % nb], future_data=None, batch_seen=i, epoch=1)
        return masked_mae_native(recon.transpose(1, 2), label.transpose(1, 2), 0.0, rescale=(MEAN, STD))
    return model, opt, micro


def separate(model, opt, micro, k, base):
    for j in range(k):
        opt.zero_grad()
        micro(base + j).backward()
        opt.step()


def group(model, opt, micro, k, base):
    opt.zero_grad()
    for j in range(k):
        (micro(base + j) / k).backward()
    opt.step()


def timed(fn, *args):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn(*args)
    e1.record()
    e1.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)


def summary(xs, k):
    q = statistics.quantiles(xs, n=10)
    med = statistics.median(xs)
    return {"per_optimizer_step_ms": med, "per_micro_batch_ms": med / k, "p10_p90_ms": [q[0], q[-1]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C4,C5,C3")
    ap.add_argument("--ks", default="1,2,4")
    ap.add_argument("--matmul", default="bf16", choices=["f32", "bf16"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_accum: needs a GPU (nothing is measured without one)")
    ks = [int(x) for x in a.ks.split(",")]
    rows = []
    for c in a.configs.split(","):
        name = NAMES[c]
        cfg = bench.CONFIGS[name]
        model, opt, micro = (pretrain_problem if cfg.get("pretrain") else step_problem)(cfg, a.matmul, max(ks) * 2)
        for k in ks:
            res = {"separate": {"host": [], "device": []}, "group": {"host": [], "device": []}}
            for r in range(a.warmup + a.rounds):
                for label, fn, kk in (("separate", separate, 1), ("group", group, k)):
                    opt.zero_grad()
                    model.set_grad_accumulation(kk)
                    h, d = timed(fn, model, opt, micro, k, r * k)
                    if r >= a.warmup:
                        res[label]["host"].append(h)
                        res[label]["device"].append(d)
            row = {"config": c, "name": name, "N": cfg["N"], "B": cfg["B"], "k": k, "matmul": a.matmul,
                   **{label: {clock: summary(v[clock], k) for clock in ("host", "device")} for label, v in res.items()}}
            row["group_over_separate_device"] = row["group"]["device"]["per_optimizer_step_ms"] / row["separate"]["device"]["per_optimizer_step_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        opt.zero_grad()
        model.set_grad_accumulation(1)
        del model, opt, micro
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_grad_accum.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup": a.warmup,
           "what": "k micro-batches as k separate k = 1 optimizer steps vs one accumulation group; medians over rounds, the two loops "
                   "alternating; host = perf_counter around a round on an idle device, device = two events; no look-ahead prefetch",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    print("| config | k | separate: ms / optimizer step (ms / micro-batch) | group | group / separate |")
    print("|---|---|---|---|---|")
    for r in rows:
        s, g = r["separate"]["device"], r["group"]["device"]
        print(f"| {r['config']} {r['name']} (B = {r['B']}) | {r['k']} | {s['per_optimizer_step_ms']:.2f} ({s['per_micro_batch_ms']:.2f}) | "
              f"{g['per_optimizer_step_ms']:.2f} ({g['per_micro_batch_ms']:.2f}) | {r['group_over_separate_device']:.3f} |")


if __name__ == "__main__":
    main()
