"""``STEP.eval_noise = "window"`` at the module level: the N = 37, L = 288 model of tests/test_gpu_eval_cache.py in bf16 mode, nine windows.

The sampled adjacency of a window (``model._last["sampled_adj"]``, which every forward has always filled) must be the same bits whatever
batch the window sits in, in whatever order, however many forwards came before, with the evaluation cache on or off.

Predictions under regrouping.  Measured on the parent commit on an MI355X with EXPLICIT noise (``_noise_override``, a per-batch stack of
per-window ``u``: the code path this change does not touch), the same nine windows in batches of 1, 4 and 9: the largest relative L2
between two groupings of the same window was 0.0 -- every window's prediction had the same bits in all three groupings, and the same
grouping twice gave the same bits (this tree, same session: 0.0 as well).  The rule: 0 -> ``torch.equal``; otherwise the bound would be
4 x that value rounded up to a power of two.  So REGROUP_BOUND = 0: the window-keyed pass must give every window the same bits in
every batching, and the explicit-noise regrouping is measured again here and held to the same.
"""
import pytest
import torch

from tests.test_gpu_eval_cache import BATCHES, _bytes, _fresh, _reseed

pytestmark = pytest.mark.gpu

ORIGINS = [t for b in BATCHES for t in b]
N = 37
REGROUP_MEASURED = 0.0          # largest relative L2 between groupings, explicit noise, parent commit (see the docstring)
REGROUP_BOUND = 0               # 0: torch.equal


def _groups(size, order=None):
    order = list(range(9)) if order is None else list(order)
    return [order[a:a + size] for a in range(0, 9, size)]


def _pass(model, loader, groups, noise=None):
    """-> window index -> (sampled adjacency [N, N], prediction [12, N, 1]) of one eval pass over the nine windows in these batches"""
    out = {}
    with torch.no_grad():
        for idx in groups:
            if noise is not None:
                model._noise_override = noise[idx].contiguous()
            hist, ref, _f = loader.batch([ORIGINS[i] for i in idx])
            pred = model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=None, epoch=None)[0]
            adj = model._last["sampled_adj"]
            for j, i in enumerate(idx):
                out[i] = (adj[j].clone(), pred[j].clone())
    model._noise_override = None
    return out


def _window_model():
    model, loader = _fresh("bf16")
    model.eval_noise = "window"
    return model, loader


def _same_adjacency(a, b):
    return all(torch.equal(a[i][0], b[i][0]) for i in range(9))


def _rel_l2(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


def _held(a, b, what):
    worst = max(_rel_l2(a[i][1], b[i][1]) for i in range(9))
    print(f"{what}: largest relative L2 between the two passes' predictions {worst:.3e} (bound {REGROUP_BOUND})")
    if REGROUP_BOUND == 0:
        assert all(torch.equal(a[i][1], b[i][1]) for i in range(9)), what
    else:
        assert worst <= REGROUP_BOUND, (what, worst)


def test_a_windows_graph_does_not_depend_on_its_batch():
    model, loader = _window_model()
    _reseed(model)
    by4 = _pass(model, loader, _groups(4))
    for i in range(9):
        a = by4[i][0]
        assert bool(((a == 0) | (a == 1)).all()) and float(a.diagonal().abs().max()) == 0.0 and 0.0 < float(a.mean()) < 1.0
    assert not torch.equal(by4[0][0], by4[1][0])                              # another window, another draw
    for size in (1, 9):
        other = _pass(model, loader, _groups(size))
        assert _same_adjacency(other, by4), size
        _held(other, by4, f"batches of {size} against batches of 4")
    shuffled = _pass(model, loader, _groups(4, order=[8, 3, 5, 0, 7, 1, 6, 2, 4]))
    assert _same_adjacency(shuffled, by4)
    _held(shuffled, by4, "another window order")
    # same batching, a second pass: the same bits (this shape is bit-reproducible: tests/test_gpu_eval_cache.py)
    again = _pass(model, loader, _groups(4))
    assert all(torch.equal(again[i][0], by4[i][0]) and torch.equal(again[i][1], by4[i][1]) for i in range(9))
    # ... and after training-mode forwards moved both seed counters.  Those forwards also move the BatchNorm running statistics, which
    # an eval forward reads: the buffers are put back, so that the pass sees the same weights under later counters
    state = {k: v.clone() for k, v in model.state_dict().items()}
    counters = (model._seed_ctr, model.tsformer._seed_counter)
    model.train()
    with torch.no_grad():
        for idx in _groups(4)[:2]:
            hist, ref, _f = loader.batch([ORIGINS[i] for i in idx])
            model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=0, epoch=1)
    model.eval()
    model.load_state_dict(state)
    assert model._seed_ctr > counters[0]
    later = _pass(model, loader, _groups(4))
    assert all(torch.equal(later[i][0], by4[i][0]) and torch.equal(later[i][1], by4[i][1]) for i in range(9))
    # another eval_noise_seed is another stream
    model.eval_noise_seed = 1
    assert not _same_adjacency(_pass(model, loader, _groups(4)), by4)


def test_with_the_evaluation_cache_and_the_kept_g():
    model, loader = _window_model()
    _reseed(model)
    want = _pass(model, loader, _groups(4))
    model.eval_cache_bytes = _bytes(9)
    first = _pass(model, loader, _groups(4))                                  # fills the cache, keeps g
    assert model.eval_cache_stats["windows_stored"] == 9
    second = _pass(model, loader, _groups(9))                                 # served from the cache, regrouped
    assert model.eval_cache_stats["window_hits"] == 9 and model.eval_cache_stats["g_reuses"] >= 3
    for got, what in ((first, "cache filling"), (second, "cache hits, one batch of 9")):
        assert _same_adjacency(got, want), what
        _held(got, want, what)
    assert all(torch.equal(first[i][1], want[i][1]) for i in range(9))        # same batching: the same bits


def test_explicit_noise_regrouping_is_what_was_measured():
    """the measurement behind REGROUP_BOUND, repeated: explicit per-window noise, batches of 1, 4 and 9"""
    model, loader = _fresh("bf16")
    noise = torch.rand(9, N * N, 2, generator=torch.Generator().manual_seed(99)).cuda()
    _reseed(model)
    res = {size: _pass(model, loader, _groups(size), noise) for size in (1, 4, 9)}
    worst = max(_rel_l2(res[a][i][1], res[b][i][1]) for a, b in ((1, 4), (1, 9), (4, 9)) for i in range(9))
    print(f"explicit noise, groupings 1 / 4 / 9: largest relative L2 {worst:.3e} (measured on the parent: {REGROUP_MEASURED}, bound {REGROUP_BOUND})")
    assert all(torch.equal(res[a][i][0], res[b][i][0]) for a, b in ((1, 4), (1, 9), (4, 9)) for i in range(9))      # the same u, the same graph
    if REGROUP_BOUND == 0:
        assert worst == 0.0
    else:
        assert worst <= REGROUP_BOUND
    # explicit noise keeps precedence over the window keys
    model.eval_noise = "window"
    keyed_off = _pass(model, loader, _groups(4), noise)
    assert all(torch.equal(keyed_off[i][0], res[4][i][0]) and torch.equal(keyed_off[i][1], res[4][i][1]) for i in range(9))


def test_seed_counters_move_as_under_positional_noise():
    counters = {}
    for mode in ("position", "window"):
        model, loader = _fresh("bf16")
        model.eval_noise = mode
        _reseed(model)
        _pass(model, loader, _groups(4))
        counters[mode] = (model._seed_ctr, model.tsformer._seed_counter)
    assert counters["window"] == counters["position"] == (6, 3)


def test_position_is_the_default_and_changes_nothing():
    """a module that never touches the switch against one that sets the default explicitly (and a seed the default must ignore): the
    same bits; and the window-keyed pass is a different draw"""
    untouched, loader = _fresh("bf16")
    assert untouched.eval_noise == "position"
    _reseed(untouched)
    want = _pass(untouched, loader, _groups(4))
    explicit, loader2 = _fresh("bf16")
    explicit.eval_noise, explicit.eval_noise_seed = "position", 5
    _reseed(explicit)
    got = _pass(explicit, loader2, _groups(4))
    assert all(torch.equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]) for i in range(9))
    # positional noise does depend on the batching: what the switch is for
    _reseed(untouched)
    assert not _same_adjacency(_pass(untouched, loader, _groups(9)), want)
    explicit.eval_noise = "window"
    _reseed(explicit)
    assert not _same_adjacency(_pass(explicit, loader2, _groups(4)), want)
    # a training forward ignores the switch: the same draw as the untouched module's
    for m in (untouched, explicit):
        _reseed(m)
        m.train()
        m.backend.dropout, m.tsformer.dropout_p = 0.0, 0.0
    with torch.no_grad():
        outs = []
        for m, ld in ((untouched, loader), (explicit, loader2)):
            hist, ref, _f = ld.batch([ORIGINS[i] for i in range(4)])
            m(history_data=hist, long_history_data=ref, future_data=None, batch_seen=0, epoch=1)
            outs.append(m._last["sampled_adj"].clone())
    assert torch.equal(outs[0], outs[1])


def test_refusals():
    model, loader = _window_model()
    hist, ref, _f = loader.batch(ORIGINS[:2])
    tensor = torch.zeros(2, 288, N, 3, device="cuda")
    with torch.no_grad():
        with pytest.raises(ValueError, match="DeviceWindowLoader / DeviceForecastingDataset"):
            model(history_data=hist, long_history_data=tensor, future_data=None, batch_seen=None, epoch=None)
        model.eval_noise = "batch"
        with pytest.raises(ValueError, match="eval_noise"):
            model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=None, epoch=None)
        model.eval_noise = "window"
        model.gumbel_noise = "torch_cpu"                                      # the host noise keeps precedence over the keys
        model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=None, epoch=None)
