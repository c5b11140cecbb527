"""``step_replica_digest`` alone, timed with events: the median of 200 launches at the flat parameter buffer of the pre-training TSFormer
of config C3 (667 404 floats, 2.67 MB) and of STEP_PEMS04 (22 228 324 floats, 88.9 MB: fc.weight is 100 x 16 x (13 599 - 18) of them).
One JSON line.

    python tools/replica_digest_bench.py [--reps 200]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"C3_tsformer_pretrain": 667404, "STEP_PEMS04": 22228324}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import torch
    from step_amd.comm import replica_digest
    out = {}
    for name, n in SIZES.items():
        flat = torch.randn(n, device="cuda")
        for _ in range(10):
            replica_digest(flat)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            replica_digest(flat)
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med = ms[len(ms) // 2]
        out[name] = {"floats": n, "bytes": 4 * n, "median_us": 1e3 * med, "min_us": 1e3 * ms[0], "p90_us": 1e3 * ms[int(0.9 * len(ms))],
                     "GB_per_s": 4 * n / (1e-3 * med) / 1e9}
    print(json.dumps({"kernel": "step_replica_digest", "reps": a.reps, "includes": "the 16-byte clear and the output allocation", **out}))


if __name__ == "__main__":
    main()
