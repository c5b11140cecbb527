"""The training loop of the REFERENCE's runner (easytorch Runner.train -> BaseTimeSeriesForecastingRunner.train_iters ->
TSFormerRunner.forward, unmodified sources found by oracle/reference_loader.py; tests/_shims stands in for easytorch: its loader has no
worker processes and does not pin) around step_amd.TSFormer in pre-train mode at config C3 (TSFormer_PEMS-BAY shape: N = 325, L = 2016,
batch 16, bf16 mode, dropout on), timed.  One JSON line.  The pre-training sibling of tools/runner_feed_bench.py.

    python tools/runner_pretrain_feed_bench.py --runner native --dataset device [--iters 40]

--runner native     CFG.RUNNER = step_amd.runner.native_runner(TSFormerRunner, native_pretrain=True)   (reference: TSFormerRunner as it is)
--dataset device    CFG.DATASET_CLS = step_amd.runner.DevicePretrainingDataset                          (host: the reference's PretrainingDataset)
--group-of-one      a process group of ONE rank (nccl = RCCL) and TSFormer.enable_native_data_parallel(single_rank_collectives=True): every
                    collective of the data-parallel backward is issued (arithmetically a no-op) -- what the path costs on a one-GPU box
"""
import argparse
import importlib
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DS, N, L = "PEMS-BAY", 325, 288 * 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runner", default="native", choices=["native", "reference"])
    ap.add_argument("--dataset", default="device", choices=["device", "host"])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--group-of-one", action="store_true")
    a = ap.parse_args()
    import torch
    from tests import dropin_common as DC
    from oracle.reference_loader import reference_root
    if reference_root() is None:
        print(json.dumps({"error": "reference sources not staged (tools/stage_reference.sh)"}))
        return
    from step_amd import TSFormer
    from step_amd.runner import DevicePretrainingDataset, native_runner

    class Workspace(DC.Workspace):
        """the three files TSFormer_PEMS-BAY.py's runner reads with cwd-relative paths (base_tsf_runner.py:36, 101-102), synthetic"""
        def __init__(self, root, n_train):
            self.root, self.ds = root, DS
            T = L + n_train + 64
            d = os.path.join(root, "datasets", DS)
            os.makedirs(d, exist_ok=True)
            idx = [(t - L, t, t + 12) for t in range(L, L + n_train)]
            for name, obj in (("data", {"processed_data": DC.synth_series(T, N)}), ("index", {"train": idx, "valid": idx[:2], "test": idx[:2]}),
                              ("scaler", {"func": "re_standard_transform", "args": {"mean": DC.MEAN, "std": DC.STD}})):
                with open(os.path.join(d, f"{name}_in{L}_out12.pkl"), "wb") as f:
                    pickle.dump(obj, f)

    with tempfile.TemporaryDirectory() as root, Workspace(root, a.batch * (a.iters + a.warmup + 2)):
        cfg = importlib.import_module("step.TSFormer_" + DS).CFG          # the reference's config file
        cfg.MODEL.ARCH = TSFormer
        cfg.TRAIN.DATA.BATCH_SIZE = a.batch
        cfg.TRAIN.DATA.SHUFFLE = True
        cfg["_DEVICE"] = "cuda"
        if a.runner == "native":
            cfg.RUNNER = native_runner(cfg.RUNNER, native_pretrain=True)
        if a.dataset == "device":
            cfg.DATASET_CLS = DevicePretrainingDataset
        torch.manual_seed(0)
        runner = cfg.RUNNER(cfg)
        runner.model.matmul_precision = "bf16"
        transport = None
        if a.group_of_one:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29583")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", torch.cuda.current_device()))
            runner.model.enable_native_data_parallel(single_rank_collectives=True)
            transport = "rccl" if runner.model._comm is not None else "torch.distributed"
        t, calls, inner = {}, [0], runner.train_iters

        def train_iters(epoch, iter_index, data):          # (pretrain_tail does not go through the module's __call__: no forward hook)
            if calls[0] == a.warmup:
                torch.cuda.synchronize()
                t["t0"] = time.perf_counter()
            calls[0] += 1
            return inner(epoch, iter_index, data)
        runner.train_iters = train_iters
        losses = runner.train(cfg, max_iters=a.warmup + a.iters)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t["t0"]
        print(json.dumps({"runner": a.runner, "dataset": a.dataset, "ms_per_step": 1e3 * dt / a.iters, "windows_per_s": a.batch * a.iters / dt,
                          "iters": a.iters, "batch": a.batch, "final_loss": losses[-1],
                          "optimizer": type(runner.optim).__name__, "dataset_cls": type(runner.train_data_loader.dataset).__name__,
                          "group_of_one": bool(a.group_of_one), "collectives": transport}))
        if a.group_of_one:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
