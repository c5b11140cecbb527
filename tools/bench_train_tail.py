"""The tail of one training iteration -- rescale -> slice -> loss -> backward down to dpred / dtheta -> three meters -- timed two ways on
synthetic device tensors (needs a GPU; nothing of the reference):

  (a) existing   torch rescale and ``[:, :k]`` slice, then ``step_loss_native`` and ``masked_metrics_native``: what ``native_runner`` does
                 with ``native_tail=False`` (the baseline)
  (b) train_tail one ``step_amd.step_loss.train_tail`` call on the normalised prediction and the batch's label view

at the shapes of bench.py's configs C1 (STEP_METR-LA) and C2 (STEP_PEMS04) and at PEMS-BAY's N = 325 with B = 8, for k in {1, 6, 12}.
Per tail it records the device launches (kernels, memsets and copies seen by torch's profiler, which also sees libstep_hip's), the host
microseconds to enqueue it and the device microseconds between two events around it (medians of --iters after --warmup; the two paths
alternate inside one loop; the device is idle before every timed tail).  There is no threshold: the claim to read off is "fewer launches
and no copies".

    python tools/bench_train_tail.py [--out profiles/train_tail.json]

``--null nan`` and / or ``--scaler node`` (and ``--parent-lib``) switch to another measurement, of the tail's own two launches under the
variants this tool did not have: the entry points of libstep_hip called directly (``step_train_tail`` / ``step_train_tail_nodes``) on the
same tensors at C2's shape (B = 8, H = 12, N = 307) and at N = 883, k = 12 -- the scalar / finite tail, the NaN ``null_val`` tail
(``--null nan``), the per-node tail (``--scaler node``) and, with ``--parent-lib PATH``, the scalar / finite tail of ANOTHER build of
libstep_hip (the parent commit's) loaded next to this tree's.  Device microseconds between two events around the two launches, medians
of --iters with the p10-p90 band, the variants alternating inside one loop.  No threshold for the new variants; what to read off is
whether the scalar / finite medians of the two builds lie within each other's band (``default_within_bands``).

    python tools/bench_train_tail.py --null nan --scaler node --parent-lib PATH [--out profiles/tail_scalers.json] [--merge]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                  # noqa: E402  (the config table)
from step_amd.step_loss import masked_metrics_native, step_loss_native, train_tail          # noqa: E402

MEAN, STD, H, C = 200.0, 150.0, 12, 3
SHAPES = {"C1 STEP_METR-LA": (bench.CONFIGS["STEP_METR-LA"]["B"], bench.CONFIGS["STEP_METR-LA"]["N"]),
          "C2 STEP_PEMS04": (bench.CONFIGS["STEP_PEMS04"]["B"], bench.CONFIGS["STEP_PEMS04"]["N"]),
          "PEMS-BAY N=325 B=8": (8, 325)}
KS = (1, 6, 12)


def inputs(B, N, gen):
    fut = torch.randn(B, H, N, C, generator=gen)
    fut[..., 0][torch.rand(B, H, N, generator=gen) < 0.2] = -MEAN / STD          # a fifth of the labels are a raw 0.0
    pred = fut[..., :1] + 0.1 * torch.randn(B, H, N, 1, generator=gen)
    theta = torch.rand(B, N, N, generator=gen).clamp(1e-4, 1 - 1e-4)
    prior = (torch.rand(B, N, N, generator=gen) < 0.05).float()
    return [t.cuda() for t in (pred.contiguous(), fut, theta, prior)]


def tail_existing(pred, fut, theta, prior, k):
    p = pred * STD + MEAN
    y = fut[..., :1] * STD + MEAN
    p, y = p[:, :k, :, :], y[:, :k, :, :]                      # base_tsf_runner.py:243-246 (curriculum learning on)
    loss = step_loss_native(p, y, theta, prior, 0.5, null_val=0.0)
    metrics = masked_metrics_native(p, y, 0.0)
    return (loss, metrics) + torch.autograd.grad(loss, [pred, theta])


def tail_native(pred, fut, theta, prior, k):
    loss, metrics = train_tail(pred, fut[..., :1], theta, prior, 0.5, null_val=0.0, rescale=(MEAN, STD), horizons=k)
    return (loss, metrics) + torch.autograd.grad(loss, [pred, theta])


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


def _band(xs):
    q = statistics.quantiles(xs, n=10)
    return {"device_us": statistics.median(xs), "device_us_p10_p90": [q[0], q[-1]]}


def variants_main(a):
    """the tail's two launches under (null_val, scaler) variants, and under another build of the library: see the module docstring"""
    from step_amd import _lib
    lib = _lib.lib()
    libs = {"tree": lib}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ("step_train_tail", "step_train_tail_work_doubles"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib._SIGS[name]
        libs["parent"] = parent
    gen = torch.Generator().manual_seed(0)
    nan = float("nan")
    rows = []
    for label, (B, N) in (("C2 STEP_PEMS04", SHAPES["C2 STEP_PEMS04"]), ("N=883 B=8", (8, 883))):
        pred, fut, theta, prior = inputs(B, N, gen)
        pred = pred[..., 0].contiguous()
        scale_n, shift_n = torch.full((N,), STD).cuda(), torch.full((N,), MEAN).cuda()
        scale_n *= torch.linspace(0.8, 1.25, N).cuda()
        loss, metrics = torch.empty((), device="cuda"), torch.empty(3, device="cuda")
        dp, dt = torch.empty_like(pred), torch.empty_like(theta)
        work = {k: torch.zeros(lb.step_train_tail_work_doubles(), dtype=torch.float64, device="cuda") for k, lb in libs.items()}

        def call(which, entry, scaler, null_val):
            rc = getattr(libs[which], entry)(_lib.ptr(pred), H * N, N, 1, ctypes.c_void_p(fut.data_ptr()), H * N * C, N * C, C, B, H, N, H, *scaler,
                                             null_val, _lib.ptr(theta), _lib.ptr(prior), theta.numel(), 0.5, _lib.ptr(work[which]), _lib.ptr(loss),
                                             _lib.ptr(metrics), _lib.ptr(dp), _lib.ptr(dt), _lib.stream())
            assert rc == 0, (which, entry, rc)

        variants = [("scalar_finite", ("tree", "step_train_tail", (STD, MEAN), 0.0))]
        if a.null == "nan":
            variants.append(("nan_null", ("tree", "step_train_tail", (STD, MEAN), nan)))
        if a.scaler == "node":
            variants.append(("per_node", ("tree", "step_train_tail_nodes", (_lib.ptr(scale_n), _lib.ptr(shift_n)), 0.0)))
            if a.null == "nan":
                variants.append(("per_node_nan_null", ("tree", "step_train_tail_nodes", (_lib.ptr(scale_n), _lib.ptr(shift_n)), nan)))
        if a.parent_lib:
            variants.append(("parent_scalar_finite", ("parent", "step_train_tail", (STD, MEAN), 0.0)))
        dev = {name: [] for name, _ in variants}
        values = {}
        for it in range(a.warmup + a.iters):
            for name, args in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                call(*args)
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    dev[name].append(1e3 * e0.elapsed_time(e1))
                if it == 0:
                    values[name] = (float(loss), metrics.tolist(), dp.clone())
        row = {"shape": label, "B": B, "N": N, "k": H, **{name: dict(_band(dev[name]), loss=values[name][0]) for name, _ in variants}}
        if a.parent_lib:
            t, p = row["scalar_finite"], row["parent_scalar_finite"]
            row["default_within_bands"] = bool(p["device_us_p10_p90"][0] <= t["device_us"] <= p["device_us_p10_p90"][1]
                                               and t["device_us_p10_p90"][0] <= p["device_us"] <= t["device_us_p10_p90"][1])
            row["default_same_bits_as_parent"] = bool(values["scalar_finite"][0] == values["parent_scalar_finite"][0]
                                                      and values["scalar_finite"][1] == values["parent_scalar_finite"][1]
                                                      and torch.equal(values["scalar_finite"][2], values["parent_scalar_finite"][2]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {}
    if a.merge and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out.update({"tool": "tools/bench_train_tail.py --null nan --scaler node --parent-lib ...", "device": torch.cuda.get_device_name(0),
                "iters": a.iters, "warmup": a.warmup,
                "what": "the training tail's two launches (libstep_hip entry points called directly, k = 12): device microseconds between "
                        "two events, medians and p10-p90, the variants alternating inside one loop; parent_scalar_finite is the parent "
                        "commit's build of the library loaded next to this tree's", "tail_rows": rows})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--null", choices=("zero", "nan"), default="zero", help="nan: also time the tail under a NaN null_val")
    ap.add_argument("--scaler", choices=("scalar", "node"), default="scalar", help="node: also time the per-node tail")
    ap.add_argument("--parent-lib", default=None, metavar="PATH", help="another build of libstep_hip.so whose scalar / finite tail is timed in the same loop")
    ap.add_argument("--merge", action="store_true", help="keep the other keys of an existing --out file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_tail: needs a GPU (nothing is measured without one)")
    if a.null == "nan" or a.scaler == "node" or a.parent_lib:
        a.out = a.out or os.path.join(ROOT, "profiles", "tail_scalers.json")
        return variants_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "train_tail.json")
    gen = torch.Generator().manual_seed(0)
    paths = (("existing", tail_existing), ("train_tail", tail_native))
    rows = []
    for label, (B, N) in SHAPES.items():
        pred, fut, theta, prior = inputs(B, N, gen)
        pred.requires_grad_(True)
        theta.requires_grad_(True)
        for k in KS:
            args = (pred, fut, theta, prior, k)
            ra, rb = tail_existing(*args), tail_native(*args)
            agree = {"loss_rel": abs(float(ra[0]) - float(rb[0])) / abs(float(ra[0])),
                     "dpred_rel_l2": float((ra[2] - rb[2]).norm() / ra[2].norm()), "dtheta_rel_l2": float((ra[3] - rb[3]).norm() / ra[3].norm()),
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
            row = {"shape": label, "B": B, "N": N, "k": k, "agreement": agree}
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
            print(json.dumps({k_: (v if k_ in ("shape", "B", "N", "k", "agreement") else {x: v[x] for x in ("launches", "host_us", "device_us")})
                              for k_, v in row.items()}), flush=True)
    out = {"tool": "tools/bench_train_tail.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "what": "one iteration tail (rescale, [:, :k] slice, loss, backward to dpred / dtheta, three meters); medians; host_us is the "
                   "time to enqueue, device_us the time between two events around the tail on an idle device", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    print("| shape | k | launches existing -> train_tail | host us | device us |")
    print("|---|---|---|---|---|")
    for r in rows:
        e, t = r["existing"], r["train_tail"]
        print(f"| {r['shape']} (B = {r['B']}) | {r['k']} | {e['launches']} -> {t['launches']} | {e['host_us']:.0f} -> {t['host_us']:.0f} | "
              f"{e['device_us']:.0f} -> {t['device_us']:.0f} |")


if __name__ == "__main__":
    main()
