"""Host side of the window-keyed eval noise and the evaluation passes spread over ranks (no GPU): the chunk rule, the Philox restatement
the GPU test relies on, the counter layout, the statistics the GPU test asserts (checked here on the float64 oracle's sample under the
restated noise, with the GPU test's seeds and keys), the runner's keywords and the ABI surface."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import edges_keyed_host as K
from tests.enc_dropout_host import philox4x32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_rank_chunks_partitions_every_chunk_exactly_once():
    from step_amd.evaluate import eval_rank_chunks
    for world in range(1, 9):
        for n in range(0, 21):
            shares = [eval_rank_chunks(n, r, world) for r in range(world)]
            assert sorted(c for s in shares for c in s) == list(range(n)), (world, n)
            assert all(s == sorted(s) and all(c % world == r for c in s) for r, s in enumerate(shares))
            assert max(len(s) for s in shares) - min(len(s) for s in shares) <= 1
    assert eval_rank_chunks(5, 0, 2) == [0, 2, 4] and eval_rank_chunks(5, 1, 2) == [1, 3] and eval_rank_chunks(3, 0, 1) == [0, 1, 2]
    for bad in ((3, 2, 2), (3, -1, 2), (3, 0, 0), (-1, 0, 1)):
        with pytest.raises(ValueError):
            eval_rank_chunks(*bad)


def test_philox_restatement_passes_the_known_answer_vectors():
    for counter, key, want in K.KNOWN_ANSWERS:
        got = philox4x32(np.array([counter], dtype=np.uint32), key[0], key[1])[0]
        assert [int(x) for x in got] == list(want), ([hex(int(x)) for x in got], [hex(x) for x in want])


def test_counter_layout_keeps_the_position_and_window_streams_apart():
    N, seed = 5, 0x0123456789ABCDEF
    E = N * N
    w = K.window_counters(N, (7 << 32) | 3)
    assert w.shape == (E, 4) and list(w[0]) == [0, 3, 7, 0x5EEE] and list(w[E - 1]) == [E - 1, 3, 7, 0x5EEE]
    p = K.position_counters(N, 3)
    assert list(p[0]) == [0, 0, 3, 0x5EED] and list(p[E - 1]) == [E - 1, 0, 3, 0x5EED]
    # no counter of one stream is a counter of the other, whatever the keys and positions: the tag word differs
    every_w = np.concatenate([K.window_counters(N, k) for k in (0, 1, 3, 1 << 32, (3 << 32), 0x5EED, (0x5EED << 32) | 0x5EED)])
    every_p = np.concatenate([K.position_counters(N, b) for b in range(8)])
    assert not set(map(tuple, every_w.tolist())) & set(map(tuple, every_p.tolist()))
    assert set(every_w[:, 3].tolist()) == {K.TAG_WINDOW} and set(every_p[:, 3].tolist()) == {K.TAG_POSITION}
    # ... and the streams themselves differ where everything but the tag agrees (key = 0 against position 0: c1 = c2 = 0)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    assert not np.array_equal(philox4x32(K.window_counters(N, 0), k0, k1), philox4x32(K.position_counters(N, 0), k0, k1))
    # keys: the low and the high word are separate counter words; equal keys are one stream
    u = K.keyed_uniform([5, 5, 5 + (1 << 32), 6], N, seed)
    assert u.shape == (4, E, 2) and u.dtype == torch.float32
    assert torch.equal(u[0], u[1]) and not torch.equal(u[0], u[2]) and not torch.equal(u[0], u[3])
    assert not torch.equal(u, K.keyed_uniform([5, 5, 5 + (1 << 32), 6], N, seed + 1))
    assert float(u.min()) >= 0.0 and float(u.max()) <= 1.0 - 2.0 ** -24
    assert bool(((u * 2.0 ** 24) == (u * 2.0 ** 24).round()).all())          # 24-bit uniforms


@pytest.mark.parametrize("B,N", K.STAT_SHAPES)
def test_chosen_seeds_and_keys_pass_the_statistics_on_the_host(B, N):
    """the GPU test's statistics with its seeds and keys, on [a0 >= 0] of the float64 oracle under the restated noise: a sample that
    differs from the device's at ties of the margin only"""
    from tests import direct_ref as D
    c = D.cached_edge_case(B, N)
    keys = K.keys_of(B)
    eye = torch.eye(N, dtype=torch.bool)
    out = []
    for seed in K.STAT_SEEDS:
        r = D.edges_ref(torch.float64, c["ep"], c["g"], K.keyed_uniform(keys, N, seed))
        out.append((r["theta"].detach(), ((r["a0"].detach() >= 0) & ~eye).double()))
    assert not torch.equal(out[0][1], out[1][1])
    K.check_statistics(out[0][0], out[0][1], out[1][0], out[1][1], keys, tag=f"host B={B} N={N}")


def test_the_direct_tests_keys_cover_the_cases():
    every = [k for ks in K.KEYS.values() for k in ks]
    assert 0 in every and any(k >= 1 << 32 for k in every)
    assert any(len(set(ks)) < len(ks) for ks in K.KEYS.values())
    assert K.KEYS[8][5] not in K.KEYS[8][:5] + K.KEYS[8][6:]          # the key of the invariance test sits once in its batch


def test_runner_keywords():
    from step_amd.runner import native_runner
    from tests.eval_runner_double import EvalRunnerDouble
    sig = inspect.signature(native_runner).parameters
    assert sig["eval_noise"].default == "position" and sig["native_test"].default is False and sig["spread_eval"].default is False
    for value in ("position", "window"):
        native_runner(EvalRunnerDouble, eval_noise=value)
    for bad in ("batch", None, "", 1):
        with pytest.raises(ValueError, match="eval_noise"):
            native_runner(EvalRunnerDouble, eval_noise=bad)
    # spread_eval without native_data_parallel (and in a single process): a documented no-op
    assert "Without ``native_data_parallel``" in native_runner.__doc__
    cls = native_runner(EvalRunnerDouble, spread_eval=True, native_eval=True, native_test=True, eval_noise="window")

    class _NoModel(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    runner = cls({"model": _NoModel(), "loss": None, "scaler": (0.0, 1.0), "cl": None})
    runner.init_training({})
    assert runner._spread_acting is False and runner._dp_acting is False and runner._helper_loaders == {}


def test_module_switch_defaults_and_values():
    """the module's switch: the default is today's behaviour; forward() refuses another value and a plain tensor (GPU tests); here the
    attributes and the fixed seed"""
    from tests.test_abi_and_host import _tiny_model
    model, _g = _tiny_model()
    assert model.eval_noise == "position" and model.eval_noise_seed == 0 and model._eval_seed_override is None
    ctr = model._seed_ctr
    a = model.eval_seed()
    assert a == model.eval_seed() and model._seed_ctr == ctr          # fixed: not from the counter, and it does not move it
    model.eval_noise_seed = 1
    assert model.eval_seed() != a
    model._eval_seed_override = 77
    assert model.eval_seed() == 77
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(torch.initial_seed() + 1)
        model._eval_seed_override, model.eval_noise_seed = None, 0
        assert model.eval_seed() != a          # derived from torch.initial_seed(), as _next_seed is


def test_header_and_binding_carry_the_keyed_entry_point():
    from step_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "step_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+step_dgl_edges_forward_keyed\s*\(([^)]*)\)", code)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[4] == "const long* key" and args[5] == "uint64_t seed"
    res, argtypes = _lib._SIGS["step_dgl_edges_forward_keyed"]
    assert len(argtypes) == 11 and "step_dgl_edges_forward_keyed" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "step_dgl_edges_forward_keyed") and _lib.ABI_VERSION == 10
    assert "0x5EEE" in hdr


def test_evaluate_refuses_a_spread_pass_before_any_collective():
    """no process group is initialised here: a collective would raise something else than ValueError"""
    from step_amd.evaluate import evaluate_pass

    class _M:
        eval_noise = "position"

    group = object()
    with pytest.raises(ValueError, match="window"):
        evaluate_pass(_M(), None, [1], process_group=group)
    _M.eval_noise = "window"
    with pytest.raises(ValueError, match="return_predictions"):
        evaluate_pass(_M(), None, [1], process_group=group, return_predictions=True)
