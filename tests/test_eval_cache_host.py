"""Evaluation cache, host side (no GPU): the bit layout of the stored prior in numpy, slot assignment and the budget, the
hit rule, every invalidation trigger of STEP.eval_cache_bytes, the host identity of a window (LongHistoryRef.t0_host), the
runner option.  The kernels and the module on the device: tests/test_gpu_eval_cache.py."""
import numpy as np
import pytest
import torch

from tests.eval_cache_bits import pack_prior_bits, unpack_prior_bits


# ---------------------------------------------------------------------------------------------- bit layout
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 307])
def test_bit_layout_definition(N):
    rng = np.random.default_rng(N)
    adj = (rng.random((2, N, N)) < 0.3).astype(np.float32)
    adj[0, N - 1, N - 1] = 1.0
    words = pack_prior_bits(adj)
    W = (N + 31) // 32
    assert words.shape == (2, N, W) and words.dtype == np.dtype("<u4")
    for (s, i, j) in [(0, 0, 0), (0, N - 1, N - 1), (1, N // 2, N // 3), (1, 0, N - 1)]:
        assert int((words[s, i, j // 32] >> np.uint32(j % 32)) & 1) == int(adj[s, i, j] != 0)          # bit b of word w <-> column 32 w + b
    if N % 32:
        assert not (words[..., W - 1] >> np.uint32(N % 32)).any()          # bits of columns >= N are 0
    assert np.array_equal(unpack_prior_bits(words, N), adj)
    assert int(sum(bin(int(w)).count("1") for w in words.reshape(-1))) == int(adj.sum())


# ---------------------------------------------------------------------------------------------- slots and budget
class _Recorder:
    """stands in for the device allocation of a storage chunk: records (windows, N)"""

    def __init__(self):
        self.calls = []

    def __call__(self, windows, N):
        self.calls.append((windows, N))
        return ("last%d" % len(self.calls), "bits%d" % len(self.calls))


def _keys(origins, series_id=1, version=0, channel=0):
    return [(series_id, version, channel, t) for t in origins]


def test_slot_assignment_budget_and_hit_rule():
    from step_amd.step_arch.eval_cache import FrozenBranchCache, window_bytes
    N = 37
    assert window_bytes(N) == 37 * 96 * 4 + 37 * 2 * 4 and window_bytes(307) == 117888 + 12280
    rec = _Recorder()
    budget = 5 * window_bytes(N) + window_bytes(N) - 1          # fits five windows, not six
    c = FrozenBranchCache(budget, N, tie="tie", alloc=rec, chunk_windows=4)
    assert c.bytes_held == 0 and rec.calls == []                # storage is allocated as windows arrive
    a, b, d = _keys([300, 288, 311]), _keys([299, 320, 301]), _keys([350])
    assert not c.is_hit(a) and c.lookup(a) == [None, None, None]
    slots, stored, refused = c.assign(a)
    assert (slots, stored, refused) == ([0, 1, 2], 3, 0) and rec.calls == [(4, N)]
    assert c.is_hit(a) and c.is_hit(list(reversed(a))) and not c.is_hit(a + b[:1]) and not c.is_hit([])
    slots, stored, refused = c.assign(b)                        # second chunk: what the budget leaves, one window
    assert (slots, stored, refused) == ([3, 4, -1], 2, 1) and rec.calls == [(4, N), (1, N)]
    assert c.bytes_held == 5 * window_bytes(N) <= budget
    assert c.assign(d) == ([-1], 0, 1) and len(rec.calls) == 2  # nothing evicted, nothing allocated: 5 of 7 stored, 2 refused
    assert not c.is_hit(b) and c.is_hit(b[:2]) and not c.is_hit(d)          # a batch is a hit only when ALL its windows are stored
    assert c.assign(a) == ([-1, -1, -1], 0, 0)                  # already stored: nothing to write, nothing refused
    # slots in arbitrary order; a batch that straddles the two chunks is one plan entry per chunk, the other samples skipped (-1)
    mixed = [b[1], a[0], b[0], a[2]]
    assert c.lookup(mixed) == [4, 0, 3, 2]
    assert c.plan(c.lookup(mixed)) == [(0, [-1, 0, 3, 2]), (1, [0, -1, -1, -1])]
    assert c.plan([-1, None, -1]) == []
    # other series, version or channel: other windows
    for other in (_keys([300], series_id=2), _keys([300], version=1), _keys([300], channel=2)):
        assert not c.is_hit(other)
    # a budget below one window stores nothing
    z = FrozenBranchCache(window_bytes(N) - 1, N, "tie", rec, 4)
    assert z.assign(a) == ([-1, -1, -1], 0, 3) and len(rec.calls) == 2 and z.bytes_held == 0


# ---------------------------------------------------------------------------------------------- host identity of a window
class _FakeDeviceTensor:
    """what LongHistoryRef's constructor asks of a device tensor, without a device"""
    is_cuda = True
    _version = 0

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


def test_t0_host_survives_feature_selection_and_device_only_origins_have_no_key():
    from step_amd.step_arch.step import LongHistoryRef
    from step_amd.step_arch.eval_cache import window_keys
    data = _FakeDeviceTensor((400, 37, 3), torch.float32)
    t0 = _FakeDeviceTensor((3,), torch.int64)
    ref = LongHistoryRef(data, t0, 288, t0_host=np.array([300, 17, 311]))
    assert ref.t0_host == (300, 17, 311) and all(type(t) is int for t in ref.t0_host)
    sel = ref[:, :, :, [0]]
    assert sel.t0_host == (300, 17, 311) and sel.channels == [0] and sel.shape == (3, 288, 37, 1)
    assert ref[:, :, :, 1:3].t0_host == (300, 17, 311)
    assert window_keys(sel) == [(id(data), 0, 0, 300), (id(data), 0, 0, 17), (id(data), 0, 0, 311)]
    assert window_keys(ref[:, :, :, [2, 0]])[0] == (id(data), 0, 2, 300)          # the channel the TSFormer reads is part of the key
    data._version = 3
    assert window_keys(sel)[0] == (id(data), 3, 0, 300)                           # ... and so is the series' version
    dev_only = LongHistoryRef(data, t0, 288)
    assert dev_only.t0_host is None and dev_only[:, :, :, [0]].t0_host is None
    assert window_keys(dev_only) is None and window_keys(torch.zeros(3, 288, 37, 1)) is None
    with pytest.raises(AssertionError):
        LongHistoryRef(data, t0, 288, t0_host=[1, 2])


# ---------------------------------------------------------------------------------------------- the module's rules
class _Ref:
    def __init__(self, data, origins):
        self.data, self.t0_host, self.channels = data, tuple(origins), [0, 1, 2]


def _model():
    from tests.test_abi_and_host import _tiny_model
    model, g = _tiny_model()
    N, L = int(g["meta"][0]), int(g["meta"][1])
    model._eval_cache_alloc = _Recorder()
    return model, N, L // 12


def test_cache_is_off_by_default_and_active_only_in_eval_without_gradients():
    model, N, P = _model()
    assert model.eval_cache_bytes == 0 and model._eval_cache is None
    assert set(model.eval_cache_stats) == {"window_hits", "window_misses", "windows_stored", "windows_refused", "invalidations", "g_reuses"}
    assert not any(model.eval_cache_stats.values())
    model.eval()
    with torch.no_grad():
        assert not model._eval_cache_active()                   # budget 0: off
        model.eval_cache_bytes = 1 << 20
        assert model._eval_cache_active()
        model.train()
        assert not model._eval_cache_active()                   # training mode
        model.eval()
    assert not model._eval_cache_active()                       # gradients could be taken
    for p in model.parameters():
        p.requires_grad_(False)
    assert model._eval_cache_active()                           # ... unless no parameter requires one
    model.discrete_graph_learning._shard = {"world": 2}
    assert not model._eval_cache_active()                       # a time-sliced graph learner keeps its own evaluation rules
    model.discrete_graph_learning._shard = None


def _stored(model, N, P, origins=(300, 288, 311)):
    ref = _Ref(torch.zeros(4, N, 3), origins)
    plan = model._eval_cache_plan(ref, N, P)
    plan["cache"].assign(plan["keys"], ref.data)
    again = model._eval_cache_plan(ref, N, P)
    assert again["hit"] and again["cache"] is plan["cache"] and plan["cache"].series[id(ref.data)] is ref.data
    return ref


TRIGGERS = ["version", "address", "operand", "range_guard", "patches", "k", "N", "load_state_dict", "_apply", "load_pre_trained_model",
            "budget"]


@pytest.mark.parametrize("trigger", TRIGGERS)
def test_every_invalidation_trigger_drops_the_stored_windows(trigger):
    model, N, P = _model()
    model.eval()
    model.eval_cache_bytes = 1 << 20
    ref = _stored(model, N, P)
    model._eval_g = ("key", torch.zeros(1))
    assert model.eval_cache_stats["invalidations"] == 0
    ts = model.tsformer
    N2, P2 = N, P
    with torch.no_grad():
        if trigger == "version":
            ts.encoder_norm.weight.add_(0.0)                    # any TSFormer parameter's version ...
        elif trigger == "address":
            q = ts.encoder.transformer_encoder.layers[2].linear1.bias
            q.data = q.data.clone()                             # ... or address
        elif trigger == "operand":
            ts.encoder_operand = "bf16"
        elif trigger == "range_guard":
            ts._range_forced_bf16 = True                        # encoder_operand_in_use
        elif trigger == "patches":
            P2 = P + 1
        elif trigger == "k":
            model.discrete_graph_learning.k += 1
        elif trigger == "N":
            N2 = N + 1
        elif trigger == "load_state_dict":
            model.load_state_dict(model.state_dict())
        elif trigger == "_apply":
            model.float()
        elif trigger == "load_pre_trained_model":
            model.load_pre_trained_model()
        elif trigger == "budget":
            model.eval_cache_bytes = 1 << 21
    if trigger in ("load_state_dict", "_apply", "load_pre_trained_model"):
        assert model._eval_cache is None and model._eval_g is None         # dropped at once, the kept g with it
    plan = model._eval_cache_plan(ref, N2, P2)
    assert not plan["hit"] and not plan["cache"].slots and model.eval_cache_stats["invalidations"] == 1
    # ... and an unchanged module keeps its windows
    plan["cache"].assign(plan["keys"], ref.data)
    assert model._eval_cache_plan(ref, N2, P2)["hit"] and model.eval_cache_stats["invalidations"] == 1


def test_kept_global_feature_is_dropped_where_weights_change_without_a_version_bump():
    model, N, P = _model()
    model.eval()
    model.eval_cache_bytes = 1 << 20
    _stored(model, N, P)
    key = model._eval_g_key(0, N, 100)
    model._eval_g = (key, torch.zeros(1))
    assert model._eval_g_lookup(key) is model._eval_g[1] and model.eval_cache_stats["g_reuses"] == 1
    assert model._eval_g_key(1, N, 100) != key                  # the precision mode is part of the key
    with torch.no_grad():
        model.discrete_graph_learning.bn2.running_var.mul_(1.0)
    assert model._eval_g_key(0, N, 100) != key                  # ... and every tensor of the learner (address and version)
    assert model._eval_g_lookup(model._eval_g_key(0, N, 100)) is None and model._eval_g is None
    for drop in (lambda: model.train(True), model._drop_eval_g, lambda: model.load_state_dict(model.state_dict()), lambda: model.double().float(),
                 model.clear_eval_cache):
        model._eval_g = (key, torch.zeros(1))
        drop()
        assert model._eval_g is None
    model.eval()
    # train() / eval() alone leaves the stored windows (they depend on the frozen TSFormer only); clear_eval_cache() drops them
    ref = _stored(model, N, P, origins=(5, 6))
    model.train()
    model.eval()
    assert model._eval_cache_plan(ref, N, P)["hit"]
    model.clear_eval_cache()
    assert model._eval_cache is None and not model._eval_cache_plan(ref, N, P)["hit"]
    # a batch without host origins has no plan: it runs as if the cache were off
    assert model._eval_cache_plan(torch.zeros(2, P * 12, N, 1), N, P) is None
    ref.t0_host = None
    assert model._eval_cache_plan(ref, N, P) is None


def test_fused_adam_clip_step_drops_the_kept_global_feature(monkeypatch):
    """FusedAdamClip.step writes the parameters through raw pointers (no version bump): it must call STEP._drop_eval_g.  The library
    call is stubbed, so this runs without a device; the native backward's call is covered on the GPU (g_reuses after a step)."""
    from step_amd import optim
    model, N, P = _model()
    calls = []
    monkeypatch.setattr(optim._lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(optim._lib, "ptr", lambda t: None)
    monkeypatch.setattr(optim._lib, "stream", lambda: None)
    opt = optim.FusedAdamClip(model, param_grads=False)
    model._flat_grad = torch.zeros_like(opt.flat)
    model._backward_count = 1
    model._eval_g = ("key", torch.zeros(1))
    opt.step()
    assert model._eval_g is None and calls == ["step_adam_clip_sharded"]


def test_native_runner_sets_the_budget_for_validation_and_test_only():
    from tests.test_abi_and_host import _DummyBase, _tiny_model
    from step_amd.runner import native_runner

    class Base(_DummyBase):
        def __init__(self, cfg):
            super().__init__(cfg)
            self.model = cfg["model"]

    model, _ = _tiny_model()
    ds = torch.utils.data.TensorDataset(torch.arange(12.0).view(6, 2), torch.arange(12.0).view(6, 2) * 0.5)
    r = native_runner(Base)({"model": model})
    r.build_train_data_loader({"dataset": ds})
    r.build_val_data_loader({})
    r.build_test_data_loader({})
    assert model.eval_cache_bytes == 0                          # the default stays off
    r = native_runner(Base, eval_cache_bytes=1 << 30)({"model": model})
    r.build_train_data_loader({"dataset": ds})
    assert model.eval_cache_bytes == 0
    r.build_val_data_loader({})
    assert model.eval_cache_bytes == 1 << 30
    model.eval_cache_bytes = 0
    r.build_test_data_loader({})
    assert model.eval_cache_bytes == 1 << 30


def test_plan_keys_on_the_channel_the_branch_reads():
    """STEP.prefetch(ref, channel=c) computes channel c of the announced reference: its plan must look the windows up under that channel"""
    model, N, P = _model()
    model.eval()
    model.eval_cache_bytes = 1 << 20
    ref = _Ref(torch.zeros(4, N, 3), (300, 288))
    assert [k[2] for k in model._eval_cache_plan(ref, N, P)["keys"]] == [0, 0]
    plan = model._eval_cache_plan(ref, N, P, channel=2)
    assert [k[2] for k in plan["keys"]] == [2, 2]
    plan["cache"].assign(plan["keys"], ref.data)
    assert model._eval_cache_plan(ref, N, P, channel=2)["hit"] and not model._eval_cache_plan(ref, N, P)["hit"]
