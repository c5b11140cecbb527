"""Host side of data-parallel training through ``native_runner`` (no GPU): the numpy restatement of ``step_replica_digest`` pinned to
hand-computed values (it is the oracle of tests/test_gpu_replica_digest.py), the runner's decision logic without a process group and
with two CPU ranks (tests/dp_host_worker.py around tests/dp_double.py), and the per-rank dropout seed streams."""
import inspect
import os
import subprocess
import sys
import warnings

import numpy as np
import torch

from tests.digest_ref import as_int64_pair, digest
from tests.test_abi_and_host import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def mix_by_hand(z):
    """splitmix64's finaliser on a Python integer, written out independently of tests/digest_ref.py"""
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_digest_reference_is_pinned_to_hand_computed_values():
    # n = 1, bits 0 at index 0: the hashed word is 0 and the finaliser maps 0 to 0
    assert digest(np.zeros(1, np.float32)) == (0, 0)
    # n = 1, 1.0f = 0x3F800000 at index 0
    one = 0x2A5CF130132EA644
    assert mix_by_hand(0x3F800000) == one
    assert digest(np.ones(1, np.float32)) == (one, one)
    # n = 2: 1.0f at index 0, -2.0f = 0xC0000000 at index 1 -> the word (1 << 32) | 0xC0000000
    two = 0x92A5BFC96934FBBA
    assert mix_by_hand((1 << 32) | 0xC0000000) == two
    assert digest(np.array([1.0, -2.0], np.float32)) == (0xBD02B0F97C63A1FE, 0xB8F94EF97A1A5DFE) == ((one + two) & M64, one ^ two)
    # position matters, and so does the sign of zero
    assert digest(np.array([-2.0, 1.0], np.float32)) != digest(np.array([1.0, -2.0], np.float32))
    assert digest(np.array([0.0], np.float32)) != digest(np.array([-0.0], np.float32))
    assert as_int64_pair((0xBD02B0F97C63A1FE, 5)) == [0xBD02B0F97C63A1FE - (1 << 64), 5]


def test_digest_reference_against_a_python_loop():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(257).astype(np.float32)
    v[3], v[100], v[200] = np.nan, np.inf, 1e-42
    s = x = 0
    for i, b in enumerate(v.view(np.uint32).tolist()):
        m = mix_by_hand((i << 32) | b)
        s, x = (s + m) & M64, x ^ m
    assert digest(v) == (s, x)


def test_the_switches_exist_and_default_to_today():
    from step_amd.runner import native_runner
    from step_amd.step_arch.tsformer import TSFormer
    sig = inspect.signature(native_runner)
    assert sig.parameters["native_data_parallel"].default is False and sig.parameters["replica_check"].default is True
    sig = inspect.signature(TSFormer.enable_native_data_parallel)
    assert list(sig.parameters)[1:] == ["process_group", "sync_module_states", "single_rank_collectives", "collectives"]
    assert sig.parameters["collectives"].default == "auto" and sig.parameters["sync_module_states"].default is True
    from step_amd import _lib
    assert "step_replica_digest" in _lib.exported_symbols()


def test_without_a_process_group_nothing_changes(tmp_path):
    """native_data_parallel=True in a single process: the same runner state as with the switch off"""
    from step_amd import TSFormer
    from step_amd.runner import native_runner
    from tests.dp_double import DistributedPretrainRunnerDouble
    from tests.runner_double import masked_mae
    assert not torch.distributed.is_initialized()
    cfg = {"TRAIN": {"OPTIM": {"PARAM": {"lr": 1e-3, "weight_decay": 0, "eps": 1e-8, "betas": (0.9, 0.95)}},
                     "LR_SCHEDULER": {"PARAM": {"milestones": [1], "gamma": 0.5}}, "CLIP_GRAD_PARAM": {"max_norm": 5.0}}}
    state = {}
    for on in (False, True):
        torch.manual_seed(0)
        model = TSFormer(12, 1, 96, 4, 4, 0.1, 16, 0.75, 4, 1, mode="pre-train")
        with warnings.catch_warnings():
            warnings.simplefilter("error")          # and nothing to warn about
            runner = native_runner(DistributedPretrainRunnerDouble, native_data_parallel=on, native_pretrain=True)(
                {"model": model, "loss": masked_mae, "scaler": (200.0, 150.0), "cl": None, "ckpt_dir": str(tmp_path / str(on))})
            runner.init_training(cfg)
        assert runner.model is model and runner._dp_acting is False
        assert model._process_group is None and model._comm is None and model._seed_rank == 0
        state[on] = (type(runner.optim), runner.clip_grad_param, type(runner.scheduler), model._flat_param,
                     [model._next_seed() for _ in range(3)], sorted(k for k in vars(runner) if not k.startswith("__")))
    assert state[True] == state[False] and state[True][0] is torch.optim.Adam


def test_two_cpu_ranks_take_one_decision(tmp_path):
    """one attempt; a worker that hangs is killed with the other one and the test fails"""
    script = os.path.join(ROOT, "tests", "dp_host_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, script, ROOT, str(tmp_path)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and "ok" in o, o[-4000:]
