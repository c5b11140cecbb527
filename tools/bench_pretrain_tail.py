"""The tail of one TSFormer pre-training iteration -- select the masked tokens -> rescale -> masked_mae -> backward down to the decoder's
output r -> three meters -- timed two ways on synthetic device tensors (needs a GPU; nothing of the reference):

  (a) views          the views ``TSFormer.forward`` cuts from r [S, P, 12] and the packed series (a slice + reshape copy, an
                     advanced-index gather, two transposes), then ``masked_mae_native`` and ``masked_metrics_native`` on them and their
                     backward into r: what ``native_runner`` does with ``native_pretrain=False`` (the baseline, the path before
                     ``TSFormer.pretrain_tail`` existed)
  (b) pretrain_tail  the autograd function of ``TSFormer.pretrain_tail`` on r and the series in place (libstep_hip step_pretrain_tail)
                     and its backward (step_scale2)

at the shape of bench.py's config C3 (TSFormer_PEMS-BAY: N = 325, L = 2016, B = 16, so S = 5200 sequences of P = 168 tokens, 126 of them
masked) and at the tiny shape of tests/golden/tsformer_pretrain_tiny.npz.  Per tail it records the device launches (kernels, memsets and
copies seen by torch's profiler, which also sees libstep_hip's), the host microseconds to enqueue it and the device microseconds between
two events around it (medians of --iters after --warmup; the two paths alternate inside one loop; the device is idle before every timed
tail).  There is no threshold.

    python tools/bench_pretrain_tail.py [--out profiles/pretrain_tail.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                  # noqa: E402  (the config table)
from step_amd.step_arch.tsformer import _PretrainTail          # noqa: E402
from step_amd.step_loss import masked_mae_native, masked_metrics_native          # noqa: E402

MEAN, STD = 200.0, 150.0
C3 = bench.CONFIGS["TSFormer_PEMS-BAY"]
SHAPES = {"C3 TSFormer_PEMS-BAY": (C3["B"], C3["N"], C3["L"] // 12), "tiny": (2, 9, 16)}          # (B, N, P); mask ratio 0.75


def inputs(B, N, P, gen):
    S, Pm = B * N, int(P * 0.75)
    mk = torch.randperm(P, generator=gen)[:Pm].sort().values
    series = torch.randn(S, P, 12, generator=gen)
    series[torch.rand(S, P, 12, generator=gen) < 0.2] = -MEAN / STD          # a fifth of the labels are a raw 0.0
    r = torch.randn(S, P, 12, generator=gen)
    r[:, P - Pm:, :] = series[:, mk, :] + 0.1 * torch.randn(S, Pm, 12, generator=gen)
    return r.cuda().requires_grad_(True), series.view(S, P * 12).cuda(), mk.int().cuda(), (B, N, P, P - Pm)


def tail_views(r, series, mk, dims):
    B, N, P, Pu = dims
    recon = r.view(B, N, P, 12)[:, :, Pu:, :].reshape(B, N, -1).transpose(1, 2)          # TSFormer._forward_pretrain
    label = series.view(B, N, P, 12)[:, :, mk.long(), :].reshape(B, N, -1).transpose(1, 2)
    loss = masked_mae_native(recon.transpose(1, 2), label.transpose(1, 2), rescale=(MEAN, STD))
    metrics = masked_metrics_native(recon.detach() * STD + MEAN, label * STD + MEAN, 0.0)
    return (loss, metrics) + torch.autograd.grad(loss, [r])


def tail_native(r, series, mk, dims):
    loss, metrics = _PretrainTail.apply(r, series, mk, 0.0, STD, MEAN, True)
    return (loss, metrics) + torch.autograd.grad(loss, [r])


def launches(fn, args, n=10):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            fn(*args)
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            names[e.name] = names.get(e.name, 0) + 1
    assert names, "the profiler recorded no device activity"
    return sum(names.values()) / n, {k: v / n for k, v in sorted(names.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_tail.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain_tail: needs a GPU (nothing is measured without one)")
    gen = torch.Generator().manual_seed(0)
    paths = (("views", tail_views), ("pretrain_tail", tail_native))
    rows = []
    for label, (B, N, P) in SHAPES.items():
        args = inputs(B, N, P, gen)
        ra, rb = tail_views(*args), tail_native(*args)
        agree = {"loss_rel": abs(float(ra[0].detach()) - float(rb[0].detach())) / abs(float(ra[0].detach())), "dr_rel_l2": float((ra[2] - rb[2]).norm() / ra[2].norm()),
                 "metrics_rel_max": float(((ra[1] - rb[1]).abs() / ra[1].abs()).max())}
        host = {n: [] for n, _ in paths}
        dev = {n: [] for n, _ in paths}
        for it in range(a.warmup + a.iters):
            for name, fn in paths:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                fn(*args)
                t1 = time.perf_counter()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    host[name].append(1e6 * (t1 - t0))
                    dev[name].append(1e3 * e0.elapsed_time(e1))
        row = {"shape": label, "B": B, "N": N, "P": P, "Pm": int(args[2].numel()), "agreement": agree}
        for name, fn in paths:
            try:
                n, by_name = launches(fn, args)
            except Exception as exc:          # a profiler that cannot trace this process: say so, keep the timings
                n, by_name = None, {"error": repr(exc)}
            row[name] = {"launches": n, "host_us": statistics.median(host[name]), "device_us": statistics.median(dev[name]),
                         "host_us_p10_p90": [statistics.quantiles(host[name], n=10)[0], statistics.quantiles(host[name], n=10)[-1]],
                         "device_us_p10_p90": [statistics.quantiles(dev[name], n=10)[0], statistics.quantiles(dev[name], n=10)[-1]],
                         "launches_by_name": by_name}
        rows.append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) or k == "agreement" else {x: v[x] for x in ("launches", "host_us", "device_us")})
                          for k, v in row.items()}), flush=True)
    out = {"tool": "tools/bench_pretrain_tail.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "what": "one pre-training iteration tail (masked tokens, rescale, masked_mae, backward to r, three meters); medians; host_us is "
                   "the time to enqueue, device_us the time between two events around the tail on an idle device", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    print("| shape | launches views -> pretrain_tail | host us | device us |")
    print("|---|---|---|---|")
    for r in rows:
        e, t = r["views"], r["pretrain_tail"]
        print(f"| {r['shape']} (B = {r['B']}, N = {r['N']}, P = {r['P']}) | {e['launches']} -> {t['launches']} | "
              f"{e['host_us']:.0f} -> {t['host_us']:.0f} | {e['device_us']:.0f} -> {t['device_us']:.0f} |")


if __name__ == "__main__":
    main()
