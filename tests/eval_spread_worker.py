"""Worker of tests/test_gpu_eval_spread.py: one process per rank, gloo group, every rank on cuda:0.

KIND ``evaluate``: ``STEP.evaluate(process_group=...)`` on nine and on ten windows of the step_small model (tests/test_gpu_eval_cache.py) in
batches of 4 -- three chunks, rank 0 takes two and rank 1 one, the last chunk short -- against each rank's own single-process pass; the
ranks' torch seeds differ, so the pass only agrees because rank 0's eval seed is handed over.

KIND ``runner`` / ``shard``: ``native_runner(SpreadRunnerDouble, native_data_parallel=True, native_tail=True, native_eval=True,
native_test=True, eval_noise="window", spread_eval=True[, shard_graph_learner=True])`` for STEP at the shard test's shape (N = 48,
L = 288, T_train = 701): two epochs of two iterations, each ending in ``on_epoch_end`` on both ranks, with 5 validation windows (three
batches of 2, the last short: rank 0 takes two, rank 1 one) and 7 test windows (four batches).  Rank 0's meters and lines against a
single-process ``native_eval`` + ``native_test`` pass over the same weights; the batches forwarded per rank; replicas; train mode.  KIND
``runner`` goes on with a run whose rank 1 has a test dataset that is not index-only: the vote fails, rank 0 warns, the passes stay on
rank 0.

Bound (``bound(n_terms)``): the larger of ``n_terms * 2^-52`` -- the f64 summation order of at most ``n_terms = B * H * N * chunks``
float32 terms, relative to a sum of non-negative terms -- and 4 x the spread between two single-process passes with explicit noise,
measured on the parent commit on an MI355X at both shapes: SPREAD_MEASURED = 0.0 (the two passes' predictions and tables had the same
bits at N = 37 and at N = 48; the same on this tree), so the bound is the summation order's: 4.3e-13 .. 1.2e-12 at these sizes."""
import os
import pickle
import re
import sys
import warnings

import numpy as np
import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel

ROOT, KIND, TMP = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, ROOT)
from step_amd import STEP                                                              # noqa: E402
from step_amd.comm import replicas_identical                                           # noqa: E402
from step_amd.evaluate import eval_rank_chunks                                         # noqa: E402
from step_amd.runner import DeviceForecastingDataset, LookaheadLoader, native_runner   # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
dev = torch.device("cuda:0")

SPREAD_MEASURED = 0.0          # relative spread of the table between two single-process passes, explicit noise, parent commit (both shapes)


def bound(n_terms):
    return max(n_terms * 2.0 ** -52, 4 * SPREAD_MEASURED)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def everyone(obj):
    out = [None] * world
    dist.all_gather_object(out, obj)
    return out


# =============================================================================================== KIND "evaluate"
def kind_evaluate():
    from tests.test_gpu_eval_cache import BATCHES, _fresh
    from tests.test_gpu_eval_metrics import MEAN, STD
    torch.manual_seed(100 + rank)                       # the ranks' own eval seeds differ
    model, loader = _fresh("bf16")
    group = dist.group.WORLD
    nine = [t for b in BATCHES for t in b]
    # ---- refused before any collective, on every rank (a pending collective would make the barrier below hang or mismatch)
    for kw, match in ((dict(), "window"), (dict(return_predictions=True), "return_predictions")):
        if kw:
            model.eval_noise = "window"
        try:
            model.evaluate(loader, nine, scaler=(MEAN, STD), batch_size=4, process_group=group, **kw)
        except ValueError as ex:
            assert match in str(ex), ex
        else:
            raise AssertionError(f"STEP.evaluate(process_group=..., {kw}) with eval_noise = {model.eval_noise!r} did not raise")
    dist.barrier()
    seeds = everyone(model.eval_seed())
    assert seeds[0] != seeds[1]
    for origins in (nine, nine + [320]):
        chunks = -(-len(origins) // 4)
        assert chunks == 3 and [len(eval_rank_chunks(chunks, r, world)) for r in range(world)] == [2, 1]
        forwards = []
        hook = model.register_forward_pre_hook(lambda m, a, kw: forwards.append(kw["history_data"].shape[0]), with_kwargs=True)
        model.train()                                   # the flag is restored on exit
        spread = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4, process_group=group)
        hook.remove()
        assert model.training and model._eval_seed_override is None
        model.eval()
        assert forwards == ([4, len(origins) - 8] if rank == 0 else [4]), forwards
        table = np.concatenate([spread.per_horizon.ravel(), spread.overall, spread.batch_mean])
        tables = everyone(table)
        assert np.array_equal(tables[0], tables[1]) and spread.batches == chunks          # every rank returns the same table, of all chunks
        # this rank's own single-process pass under rank 0's seed (rank 0: its own seed)
        model._eval_seed_override = seeds[0]
        single = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4)
        model._eval_seed_override = None
        want = np.concatenate([single.per_horizon.ravel(), single.overall, single.batch_mean])
        b = bound(4 * 12 * 37 * chunks)
        print(f"rank {rank} evaluate({len(origins)} windows): spread pass against the single-process pass, relative {rel(table, want):.3e} (bound {b:.3e})",
              flush=True)
        assert single.batches == chunks and rel(table, want) <= b
        if rank == 1:                                   # the control: under its OWN seed rank 1 computes another pass
            own = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4)
            assert rel(np.concatenate([own.per_horizon.ravel(), own.overall, own.batch_mean]), want) > 1e3 * b
    # ---- EvalMetrics.all_reduce with a rank that has no update
    from step_amd import EvalMetrics
    m = EvalMetrics(12, 0.0, rescale=(STD, MEAN))
    if rank == 0:
        hist, ref, fut = loader.batch(nine[:3])
        m.update(fut[..., 1:2].contiguous(), fut[..., 0:1])
        alone = m.result()
    m.all_reduce()
    r = m.result()
    assert r.batches == 1
    if rank == 0:
        assert np.array_equal(r.per_horizon, alone.per_horizon) and np.array_equal(r.batch_mean, alone.batch_mean)


# =============================================================================================== KIND "runner" / "shard"
EPOCHS, ITERS, BATCH = 2, 2, 2
N, L, T_train = 48, 288, 701
CFG = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 2e-3, "weight_decay": 1e-5, "eps": 1e-8}},
                 "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 3.0}}}
LINE = re.compile(r"^Evaluate best model on test data for horizon (\d+), Test MAE: (\d+\.\d{4}), Test RMSE: (\d+\.\d{4}), Test MAPE: (\d+\.\d{4})$")
NAMES = ("MAE", "RMSE", "MAPE")


class HostWindows(torch.utils.data.Dataset):
    """a test dataset that is NOT index-only: the reference's (future, history, long history) tensors from the host"""

    def __init__(self, prob, origins):
        self.prob, self.origins = prob, origins

    def __len__(self):
        return len(self.origins)

    def __getitem__(self, i):
        hist, long_hist, fut = self.prob.batch([self.origins[i]])
        return fut[0], hist[0], long_hist[0]


def problem():
    from tests import train_problem as TPb
    prob = TPb.Problem(N, L, T_train, n_train=32, n_eval=12)
    samples = world * ITERS * BATCH
    split = {"train": sorted(prob.train_t[:samples]), "valid": sorted(prob.eval_t[:5]), "test": sorted(prob.eval_t[5:12])}
    d = os.path.join(TMP, f"data_rank{rank}")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "data.pkl"), "wb") as f:
        pickle.dump({"processed_data": prob.series}, f)
    with open(os.path.join(d, "index.pkl"), "wb") as f:
        pickle.dump({k: [(o - 12, o, o + 12) for o in v] for k, v in split.items()}, f)
    sets = {k: DeviceForecastingDataset(os.path.join(d, "data.pkl"), os.path.join(d, "index.pkl"), k, L) for k in split}
    return prob, split, sets


def eval_loader(dataset):
    return torch.utils.data.DataLoader(dataset, batch_size=BATCH, shuffle=False)


def lines_of(log, at):
    got = [LINE.match(line) for line in log[at:at + 12]]
    assert all(m is not None for m in got) and [int(m.group(1)) for m in got] == list(range(1, 13)), log[at:at + 12]
    return np.array([[float(x) for x in m.groups()[1:]] for m in got])


def kind_runner(shard):
    from step_amd.step_loss import step_loss_native
    from tests import train_problem as TPb
    from tests.spread_double import SpreadRunnerDouble, TestPassDouble
    prob, split, sets = problem()
    val_batches = [tuple(split["valid"][a:a + BATCH]) for a in range(0, 5, BATCH)]
    test_batches = [tuple(split["test"][a:a + BATCH]) for a in range(0, 7, BATCH)]
    switches = dict(native_data_parallel=True, native_tail=True, native_eval=True, native_test=True, eval_noise="window", spread_eval=True,
                    shard_graph_learner=shard)

    def new_runner(name, test_set):
        torch.manual_seed(100 + rank)
        model = TPb.build_native(N, L, T_train, prob.series, k=5, seed=rank).to(dev)          # the ranks start apart: rank 0's state is broadcast
        model.train()
        model.matmul_precision = "bf16"
        runner = native_runner(SpreadRunnerDouble, **switches)(
            {"model": model, "loss": step_loss_native, "scaler": (prob.mean, prob.std), "cl": None, "iter_per_epoch": ITERS,
             "ckpt_dir": os.path.join(TMP, name), "dataset": sets["train"], "batch_size": BATCH})
        assert isinstance(runner.model, DistributedDataParallel)
        runner.init_training(dict(CFG, val_loader=eval_loader(sets["valid"]), test_loader=eval_loader(test_set)))
        assert runner.model is model and runner._dp_acting is True and runner._shard_acting is shard
        return runner, model

    # ------------------------------------------------------------------------------------------ the switch acts
    runner, model = new_runner("run1", sets["test"])
    assert runner._spread_acting is True and model.eval_noise == "window"
    assert len(set(everyone(model._eval_seed_override))) == 1 and model._eval_seed_override is not None          # rank 0's seed everywhere
    mine = (runner.val_data_loader, runner.test_data_loader) if rank == 0 else (runner._helper_loaders["val"], runner._helper_loaders["test"])
    assert all(isinstance(ld, LookaheadLoader) and ld.share == (rank, world) for ld in mine)
    assert (rank == 0) == (runner.val_data_loader is not None) and [len(ld) for ld in mine] == ([2, 2] if rank == 0 else [1, 2])
    for epoch in range(1, EPOCHS + 1):
        before = runner.eval_forwards
        del runner.eval_batches[:]
        path = runner.train_loader_epoch(epoch)
        assert (path is not None) == (rank == 0)
        assert model.training                                          # back in train mode on both ranks
        # every validation and test batch was forwarded exactly once over the two ranks, with the loader's composition
        assert runner.eval_forwards - before == (4 if rank == 0 else 3)
        seen = everyone(list(runner.eval_batches))
        assert seen[0] == [val_batches[0], val_batches[2], test_batches[0], test_batches[2]], seen[0]
        assert seen[1] == [val_batches[1], test_batches[1], test_batches[3]], seen[1]
    ns = model._grad_layout()["norm_slot"] if shard else None
    assert replicas_identical(model._flat_param[:ns] if shard else model._flat_param)          # the replicas stay bit-identical
    assert runner.val_base_calls == 0 and runner.test_base_calls == 0 and runner.base_calls == 0
    assert runner.eval_readbacks == (2 * EPOCHS if rank == 0 else 0)                         # one table per pass, read on rank 0 only
    if rank == 0:
        got = runner.epoch_meters[EPOCHS]
        val_calls = [(name, n) for name, _v, n in runner.meter_log if name.startswith("val_")]
        assert val_calls == [("val_" + k, 3) for k in NAMES] * EPOCHS                       # n = the batches of the WHOLE pass
        assert len(runner.logger.lines) == 12 * EPOCHS
        got_lines = lines_of(runner.logger.lines, 12 * (EPOCHS - 1))
        assert runner.val_mae_at_validating_end == got["val_MAE"]
        # ---- a single-process native_eval + native_test pass over the same weights (this process, rank 0's seed, no spread)
        ref = native_runner(TestPassDouble, native_eval=True, native_test=True, eval_noise="window")(
            {"model": model, "loss": step_loss_native, "scaler": (prob.mean, prob.std), "cl": None})
        cfg = {"val_loader": eval_loader(sets["valid"]), "test_loader": eval_loader(sets["test"])}
        ref.val_data_loader, ref.test_data_loader = ref.build_val_data_loader(cfg), ref.build_test_data_loader(cfg)
        assert ref._spread_acting is False and ref.val_data_loader.share is None
        ref.validate(train_epoch=EPOCHS)
        model.eval()
        ref.test()
        model.train()
        assert ref.eval_forwards == 7 and ref.eval_batches == val_batches + test_batches
        want = {k: m.avg for k, m in ref.meters.items()}
        want_lines = lines_of(ref.logger.lines, 0)
        b_val, b_test = bound(BATCH * 12 * N * 3), bound(BATCH * 12 * N * 4)
        for k in NAMES:
            for pre, b in (("val_", b_val), ("test_", b_test)):
                d = abs(got[pre + k] - want[pre + k]) / abs(want[pre + k])
                print(f"{KIND} {pre}{k}: spread {got[pre + k]!r}, single process {want[pre + k]!r}, relative {d:.3e} (bound {b:.3e})", flush=True)
                assert d <= b, (pre + k, d, b)
        assert abs(runner.val_mae_at_validating_end - ref.val_mae_at_validating_end) <= b_val * abs(ref.val_mae_at_validating_end)
        # the lines print four decimals: numbers within the bound of each other print within bound + 1e-4
        assert np.all(np.abs(got_lines - want_lines) <= b_test * np.abs(want_lines) + 1e-4), (got_lines, want_lines)
        first = runner.epoch_meters[1]
        assert first["val_MAE"] != got["val_MAE"]                     # two different epochs went in
    dist.barrier()
    if shard:
        return
    # ------------------------------------------------------------------------------------------ a rank that cannot: nobody spreads
    del runner, model
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        runner, model = new_runner("run2", HostWindows(prob, split["test"]) if rank == 1 else sets["test"])
    told = [w for w in caught if "spread_eval needs" in str(w.message)]
    assert len(told) == (1 if rank == 0 else 0), [str(w.message) for w in caught]
    assert runner._spread_acting is False and runner._helper_loaders == {} and model._eval_seed_override is None
    if rank == 0:
        assert runner.val_data_loader.share is None and runner.test_data_loader.share is None and model.eval_noise == "window"
    path = runner.train_loader_epoch(1)                                # nothing hangs: the passes run on rank 0 alone
    assert runner.eval_forwards == (7 if rank == 0 else 0) and model.training
    assert runner.eval_readbacks == (2 if rank == 0 else 0)
    if rank == 0:
        assert runner.eval_batches == val_batches + test_batches and len(runner.logger.lines) == 12
    assert replicas_identical(model._flat_param)


{"evaluate": kind_evaluate, "runner": lambda: kind_runner(False), "shard": lambda: kind_runner(True)}[KIND]()
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
