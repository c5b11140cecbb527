"""Worker of tests/test_gpu_eval_per_node.py: one process per rank, gloo group, every rank on cuda:0.

``STEP.evaluate(process_group=..., per_node=True)`` under ``eval_noise = "window"`` on nine windows of the step_small model
(tests/test_gpu_eval_cache.py) in batches of 4 -- three chunks, rank 0 takes two and rank 1 one -- returns the same per-node table on
both ranks, and that table is the one-process pass's under rank 0's eval seed.  Then ``EvalMetrics(nodes=N).all_reduce`` with a rank that
has no update.

Bound: relative 1e-12.  The spread pass and the one-process pass hold f64 sums of the SAME float32 terms (the predictions of the two had
the same bits on an MI355X: tests/eval_spread_worker.py) added in another order -- per (horizon, node) slot at most 9 terms, per rank
first and then over the ranks -- which moves an f64 sum of non-negative terms by a few 2^-53 of its value."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def everyone(obj):
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out


def main():
    from step_amd import EvalMetrics
    from tests.test_gpu_eval_cache import BATCHES, _fresh
    from tests.test_gpu_eval_metrics import MEAN, STD
    torch.manual_seed(100 + rank)                       # the ranks' own eval seeds differ
    model, loader = _fresh("bf16")
    model.eval_noise = "window"
    group = dist.group.WORLD
    nine = [t for b in BATCHES for t in b]
    # predictions of a spread pass stay unavailable, in data units too: refused before any collective, on every rank
    for rp in (True, "data"):
        try:
            model.evaluate(loader, nine, scaler=(MEAN, STD), batch_size=4, process_group=group, per_node=True, return_predictions=rp)
        except ValueError as ex:
            assert "return_predictions" in str(ex), ex
        else:
            raise AssertionError(f"STEP.evaluate(process_group=..., return_predictions={rp!r}) did not raise")
    dist.barrier()
    seeds = everyone(model.eval_seed())
    assert seeds[0] != seeds[1]
    forwards = []
    hook = model.register_forward_pre_hook(lambda m, a, kw: forwards.append(kw["history_data"].shape[0]), with_kwargs=True)
    spread = model.evaluate(loader, nine, scaler=(MEAN, STD), batch_size=4, process_group=group, per_node=True)
    hook.remove()
    assert forwards == ([4, 1] if rank == 0 else [4]), forwards
    assert spread.per_node.shape == (37, 12, 3) and spread.per_node_overall.shape == (37, 3) and spread.batches == 3
    table = np.concatenate([spread.per_node.ravel(), spread.per_node_overall.ravel()])
    tables = everyone(table)
    assert np.array_equal(tables[0], tables[1])          # every rank returns the whole table
    model._eval_seed_override = seeds[0]                 # this rank's own one-process pass under rank 0's seed
    single = model.evaluate(loader, nine, scaler=(MEAN, STD), batch_size=4, per_node=True)
    model._eval_seed_override = None
    want = np.concatenate([single.per_node.ravel(), single.per_node_overall.ravel()])
    assert (want > 0.0).all()
    d = rel(table, want)
    print(f"rank {rank}: per-node table of the spread pass against the one-process pass, relative {d:.3e} (bound 1e-12)", flush=True)
    assert d <= 1e-12
    assert rel(spread.per_horizon, single.per_horizon) <= 1e-12
    # ---- all_reduce with a rank that has no update: one collective over the accumulator AND the table
    m = EvalMetrics(12, 0.0, rescale=(STD, MEAN), nodes=37)
    if rank == 0:
        hist, ref, fut = loader.batch(nine[:3])
        m.update(fut[..., 1:2].contiguous(), fut[..., 0:1])
        alone = m.result()
    calls = []
    all_reduce = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: calls.append(t.numel()) or all_reduce(t, *a, **k)
    m.all_reduce()
    dist.all_reduce = all_reduce
    assert calls == [5 * 12 + 10 + 5 * 12 * 37], calls
    r = m.result()
    assert r.batches == 1
    if rank == 0:
        assert np.array_equal(r.per_node, alone.per_node) and np.array_equal(r.per_node_overall, alone.per_node_overall)


main()
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
