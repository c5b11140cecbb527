"""Evaluation cache on the device: the two kernels against the numpy definition of the bit layout, and STEP.eval_cache_bytes
against the same module with the cache off -- equality of every output, launches saved, budget, invalidation, seed neutrality,
the look-ahead loader.  Host-side rules: tests/test_eval_cache_host.py.

Equality is bit-identity wherever the uncached path is itself bit-reproducible at this shape (established first, by running
the uncached model twice); where it is not, the bound is twice the largest difference seen between the two uncached runs --
the cached model reuses one draw of the same run-to-run noise (the kept g), so its distance to either run is a difference of
two such draws.  The kNN prior comes from the bit-reproducible frozen branch and is compared exactly in every case."""
import functools
import pickle

import numpy as np
import pytest
import torch

from tests.eval_cache_bits import pack_prior_bits
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

SENTINEL_F, SENTINEL_W = -7.25, 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------- kernels alone
def _store(last, adj, slots, cache_last, cache_bits):
    from step_amd import _lib as L
    B, N = adj.shape[0], adj.shape[1]
    slot = torch.tensor(slots, dtype=torch.int64, device="cuda")
    L.call("step_frozen_cache_store", L.ptr(last), L.ptr(adj), B, N, L.ptr(slot), cache_last.shape[0], L.ptr(cache_last), L.ptr(cache_bits),
           L.stream())


def _load(cache_last, cache_bits, slots, last, adj):
    from step_amd import _lib as L
    B, N = adj.shape[0], adj.shape[1]
    slot = torch.tensor(slots, dtype=torch.int64, device="cuda")
    L.call("step_frozen_cache_load", L.ptr(cache_last), L.ptr(cache_bits), cache_last.shape[0], L.ptr(slot), B, N, L.ptr(last), L.ptr(adj),
           L.stream())


def _prior(kind, B, N, gen):
    if kind == "random":
        return (torch.rand(B, N, N, generator=gen) < 0.4).float()
    if kind == "ones":
        return torch.ones(B, N, N)
    a = torch.zeros(B, N, N)
    if kind == "corner":
        a[:, N - 1, N - 1] = 1.0
    return a


def _words(cache_bits):
    return cache_bits.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("prior", ["random", "ones", "zeros", "corner"])
@pytest.mark.parametrize("N", [33, 64, 307])
def test_store_and_load_kernels(N, prior):
    B, cap, W = 3, 5, (N + 31) // 32
    gen = torch.Generator().manual_seed(N)
    last = torch.randn(B, N, 96, generator=gen).cuda()
    adj = _prior(prior, B, N, gen).cuda()
    cache_last = torch.full((cap, N, 96), SENTINEL_F, device="cuda")
    cache_bits = torch.full((cap, N, W), SENTINEL_W, dtype=torch.int32, device="cuda")
    _store(last, adj, [4, 0, 2], cache_last, cache_bits)          # slots in arbitrary, non-monotonic order
    want = pack_prior_bits(adj.cpu().numpy())
    got = _words(cache_bits)
    for b, s in enumerate([4, 0, 2]):
        assert np.array_equal(got[s], want[b]), (N, prior, b)     # exact words, tail bits zero (pack_prior_bits pads with zeros)
        assert torch.equal(cache_last[s], last[b])
    for s in (1, 3):                                              # untouched slots still hold the sentinel
        assert (got[s] == SENTINEL_W).all() and (cache_last[s] == SENTINEL_F).all()
    last2 = torch.full((B, N, 96), float("nan"), device="cuda")
    adj2 = torch.full((B, N, N), float("nan"), device="cuda")
    _load(cache_last, cache_bits, [4, 0, 2], last2, adj2)
    assert torch.equal(last2, last) and torch.equal(adj2, adj)
    assert set(adj2.unique().tolist()) <= {0.0, 1.0}
    # one more store: the middle sample's slot is < 0 and must leave the whole cache as it is
    before_last, before_bits = cache_last.clone(), cache_bits.clone()
    other_last = torch.randn(B, N, 96, generator=gen).cuda()
    other_adj = (1.0 - adj).contiguous()
    _store(other_last, other_adj, [1, -1, 3], cache_last, cache_bits)
    want2 = pack_prior_bits(other_adj.cpu().numpy())
    got = _words(cache_bits)
    assert np.array_equal(got[1], want2[0]) and np.array_equal(got[3], want2[2])
    assert torch.equal(cache_last[1], other_last[0]) and torch.equal(cache_last[3], other_last[2])
    for s in (4, 0, 2):
        assert torch.equal(cache_bits[s], before_bits[s]) and torch.equal(cache_last[s], before_last[s])
    # ... and a load skips such a sample as well: its rows keep what they held
    last3 = torch.full((B, N, 96), SENTINEL_F, device="cuda")
    adj3 = torch.full((B, N, N), SENTINEL_F, device="cuda")
    _load(cache_last, cache_bits, [3, -1, 0], last3, adj3)
    assert torch.equal(last3[0], other_last[2]) and torch.equal(adj3[0], other_adj[2])
    assert torch.equal(last3[2], last[1]) and torch.equal(adj3[2], adj[1])
    assert (last3[1] == SENTINEL_F).all() and (adj3[1] == SENTINEL_F).all()


# ---------------------------------------------------------------------------------------------- the module
BATCHES = [[300, 288, 350], [310, 100, 388], [295, 377, 333]]          # one origin below L = 288: zero-filled history
SEED = 1234


def _series(N):
    return torch.randn(400, N, 3, generator=torch.Generator().manual_seed(11)).cuda()


def _fresh(mode, operand="f16", warm=True):
    """a model with the golden's weights in eval mode, its range guard past the launches it checks at once"""
    from step_amd import DeviceWindowLoader
    from tests.test_gpu_step import build_native
    g = load_golden("step_small")
    N, L = int(g["meta"][0]), int(g["meta"][1])
    assert (N, L, int(g["meta"][4])) == (37, 288, 4)
    model = build_native(g)
    model.matmul_precision = mode
    model.tsformer.encoder_operand = operand
    model.eval()
    loader = DeviceWindowLoader(_series(N), L)
    if warm:
        with torch.no_grad():
            for _ in range(model.tsformer.range_check_launches):
                hist, ref, _f = loader.batch(torch.tensor([200, 250, 260], device="cuda"))          # device origins: never cached
                model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=0, epoch=1)
    return model, loader


def _reseed(model):
    torch.manual_seed(SEED)
    model._seed_ctr = 0
    model.tsformer._seed_counter = 0


def _pass(model, loader, batches=BATCHES):
    out = []
    with torch.no_grad():
        for t0 in batches:
            hist, ref, _f = loader.batch(t0)
            pred, theta, knn, _c = model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=0, epoch=1)
            out.append((pred.clone(), theta.clone(), knn.clone()))
    return out


def _two_passes(model, loader):
    _reseed(model)
    return _pass(model, loader) + _pass(model, loader)


def _gap(xs, ys):
    """largest |difference| of the predictions and of theta over the batches; the kNN priors must be equal"""
    dp = max(float((x[0] - y[0]).abs().max()) for x, y in zip(xs, ys))
    dt = max(float((x[1] - y[1]).abs().max()) for x, y in zip(xs, ys))
    return dp, dt, all(torch.equal(x[2], y[2]) for x, y in zip(xs, ys))


@functools.lru_cache(maxsize=None)
def _uncached(mode, operand="f16"):
    """two uncached runs of two passes each: the reference outputs and how far the uncached path is from itself"""
    model, loader = _fresh(mode, operand)
    first = _two_passes(model, loader)
    second = _two_passes(model, loader)
    dp, dt, knn_equal = _gap(first, second)
    print(f"uncached {mode}/{operand}: run-to-run |d prediction| = {dp:.3e}, |d theta| = {dt:.3e}, kNN equal = {knn_equal}")
    assert knn_equal          # test_prefetched_frozen_branch_is_bit_identical relies on the same
    return first, (dp, dt)


def _assert_same(got, want, noise, what):
    dp, dt, knn_equal = _gap(got, want)
    print(f"{what}: |d prediction| = {dp:.3e} (uncached run-to-run {noise[0]:.3e}), |d theta| = {dt:.3e} ({noise[1]:.3e}), kNN equal = {knn_equal}")
    assert knn_equal, what
    assert dp <= 2 * noise[0] and dt <= 2 * noise[1], (what, dp, dt, noise)          # noise == 0: bit-identity


def _bytes(windows, N=37):
    from step_amd.step_arch.eval_cache import window_bytes
    return windows * window_bytes(N) + 64


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_cached_passes_equal_uncached_and_launch_nothing(mode):
    want, noise = _uncached(mode)
    if mode == "bf16":
        assert noise == (0.0, 0.0)          # this leg is exact: the bf16-mode path is bit-reproducible at this shape
    model, loader = _fresh(mode)
    model.eval_cache_bytes = _bytes(9)
    model._eval_cache_chunk_windows = 4     # chunks of 4, 4 and 1 windows: the second and third batch straddle two chunks
    model.tsformer._events = []
    st = model.eval_cache_stats
    _reseed(model)
    first = _pass(model, loader)
    assert len(model.tsformer._events) == 3
    assert (st["window_misses"], st["window_hits"], st["windows_stored"], st["windows_refused"], st["g_reuses"]) == (9, 0, 9, 0, 2)
    assert [c[2] for c in model._eval_cache.chunks] == [4, 4, 1] and model._eval_cache.bytes_held <= model.eval_cache_bytes
    second = _pass(model, loader)
    assert len(model.tsformer._events) == 3          # no encoder launch in the second pass
    assert (st["window_misses"], st["window_hits"], st["windows_stored"], st["g_reuses"], st["invalidations"]) == (9, 9, 9, 5, 0)
    assert model._last["sim"] is None and model._last["hidden_bf16"] is None
    assert model.tsformer._seed_counter == 6 and model._seed_ctr == 12          # the seeds moved as without the cache
    _assert_same(first + second, want, noise, f"cache on, {mode}")


def test_budget_of_four_windows():
    want, noise = _uncached("bf16")
    model, loader = _fresh("bf16")
    model.eval_cache_bytes = _bytes(4)
    model._eval_cache_chunk_windows = 3
    model.tsformer._events = []
    st = model.eval_cache_stats
    _reseed(model)
    first = _pass(model, loader)
    assert (st["windows_stored"], st["windows_refused"]) == (4, 5)
    assert model._eval_cache.bytes_held <= model.eval_cache_bytes
    second = _pass(model, loader)
    assert len(model.tsformer._events) == 3 + 2          # one hit batch, two computed batches
    assert (st["window_hits"], st["window_misses"], st["windows_stored"], st["windows_refused"]) == (3, 14, 4, 10)          # misses: 9 + the 2 + 3 windows not stored
    _assert_same(first + second, want, noise, "budget of 4 windows")


def test_operand_switch_misses_and_equals_an_uncached_bf16_operand_model():
    want, noise = _uncached("bf16", "bf16")
    model, loader = _fresh("bf16")
    model.eval_cache_bytes = _bytes(9)
    model.tsformer._events = []
    _two_passes(model, loader)
    assert len(model.tsformer._events) == 3 and model.eval_cache_stats["window_hits"] == 9
    model.tsformer.encoder_operand = "bf16"
    _reseed(model)
    third = _pass(model, loader)
    assert len(model.tsformer._events) == 6 and model.eval_cache_stats["invalidations"] == 1
    assert model.eval_cache_stats["window_misses"] == 18
    fourth = _pass(model, loader)
    assert len(model.tsformer._events) == 6 and model.eval_cache_stats["window_hits"] == 18
    _assert_same(third + fourth, want, noise, "after the operand switch")


# ---------------------------------------------------------------------------------------------- training steps in between
def _train_setup(cache_windows):
    from tests.test_gpu_step import inputs_of
    g = load_golden("step_small")
    model, loader = _fresh("bf16")
    model.eval_cache_bytes = _bytes(cache_windows) if cache_windows else 0
    model.tsformer._events = []
    return g, model, loader, inputs_of(g)


def _forward_backward(g, model, inputs):
    from oracle import step_oracle as O
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs
    model.train()
    model.zero_grad(set_to_none=True)
    pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=1)
    loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef)
    loss.backward()
    model.eval()
    return loss.detach().clone(), model._flat_grad.clone()


def _generator_state(model):
    """everything the dropout masks and the Gumbel noise of the next forward are drawn from"""
    return (model._seed_ctr, model.tsformer._seed_counter, torch.initial_seed(), torch.get_rng_state().tolist(), torch.cuda.get_rng_state().tolist())


@functools.lru_cache(maxsize=None)
def _seed_sequence(cache_windows):
    """train step (forward + backward; the weights stay), eval pass (cold), eval pass (warm), train step -> losses, flat gradients and
    the generator state after each of the four phases"""
    g, model, loader, inputs = _train_setup(cache_windows)
    _reseed(model)
    rec = {"loss": [], "grad": [], "state": []}
    for phase in ("train", "eval", "eval", "train"):
        if phase == "train":
            loss, grad = _forward_backward(g, model, inputs)
            rec["loss"].append(loss)
            rec["grad"].append(grad)
        else:
            _pass(model, loader)
        rec["state"].append(_generator_state(model))
    rec["hits"] = model.eval_cache_stats["window_hits"]
    return rec


def test_training_steps_draw_the_same_seeds_with_the_cache_on():
    """Deterministic parts exactly: after every phase the seed counters and torch's generators of the cached model equal the
    uncached model's, and both training losses are bit-identical (in bf16 mode the training forward is a deterministic function of the
    weights, the dropout masks and the Gumbel noise).  The native backward sums with f32 atomics, so flat gradients are compared
    in relative L2 with a fixed bound of 1e-3: summation order moves an f32 sum of n <= 1e5 terms by about sqrt(n) * 6e-8 = 2e-5 of
    the terms' magnitude, a few times more after cancellation, while another dropout mask (10 % of the encoder's activations, 30 %
    of the gcn's) or other Gumbel noise changes the gradient by a fraction of order one -- and would already show in the loss."""
    a, b = _seed_sequence(0), _seed_sequence(9)
    assert b["hits"] == 9 and a["hits"] == 0          # the warm pass of the cached run did skip its encoder launches
    for i, (x, y) in enumerate(zip(a["state"], b["state"])):
        assert x == y, f"generator state differs after phase {i}"
    for i in range(2):
        rel = float((a["grad"][i] - b["grad"][i]).norm() / a["grad"][i].norm())
        print(f"train step {i}: loss {float(a['loss'][i]):.6f} / {float(b['loss'][i]):.6f}, relative L2 of the gradient difference {rel:.3e}")
        assert torch.equal(a["loss"][i], b["loss"][i])
        assert float(a["grad"][i].norm()) > 0 and rel <= 1e-3


def test_optimizer_step_recomputes_g_and_keeps_the_stored_windows():
    """after train(), a native backward and FusedAdamClip.step, g is computed again, the stored windows still hit, and the pass equals
    the uncached path on the same stepped weights: the same model with the cache switched off, given the same seeds (bit-identity:
    the bf16-mode evaluation is bit-reproducible, test_cached_passes_equal_uncached_and_launch_nothing asserts it)"""
    from step_amd.optim import FusedAdamClip
    g, model, loader, inputs = _train_setup(9)
    opt = FusedAdamClip(model, lr=2e-3, weight_decay=1e-5, eps=1e-8, max_norm=3.0, param_grads=False)
    st, ev = model.eval_cache_stats, model.tsformer._events
    _reseed(model)
    _pass(model, loader)
    warm = _pass(model, loader)
    assert len(ev) == 3 and (st["window_misses"], st["window_hits"], st["g_reuses"]) == (9, 9, 5)
    _forward_backward(g, model, inputs)
    model.train()
    opt.step()
    model.eval()
    assert len(ev) == 4
    seeds = (model._seed_ctr, model.tsformer._seed_counter)
    cached = _pass(model, loader)
    # g computed again by the first forward (2 more reuses, not 3); no encoder launch: the frozen branch does not depend on the step
    assert len(ev) == 4 and (st["window_misses"], st["window_hits"], st["g_reuses"], st["invalidations"]) == (9, 18, 7, 0)
    model.eval_cache_bytes = 0
    model._seed_ctr, model.tsformer._seed_counter = seeds
    uncached = _pass(model, loader)
    assert len(ev) == 7 and st["window_hits"] == 18
    for x, y in zip(cached, uncached):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
    assert float((cached[0][0] - warm[0][0]).abs().max()) > 0          # the step did change what the evaluation computes


# ---------------------------------------------------------------------------------------------- the look-ahead loader
def test_lookahead_loader_hands_out_host_origins_and_a_second_iteration_is_all_hits(tmp_path):
    from step_amd.runner import DeviceForecastingDataset, LookaheadLoader
    model, _loader = _fresh("bf16")
    N, L = 37, 288
    series = _series(N).cpu().numpy()
    with open(tmp_path / "data.pkl", "wb") as f:
        pickle.dump({"processed_data": series}, f)
    origins = [t for b in BATCHES for t in b]
    idx = {k: [(t - 12, t, t + 12) for t in origins] for k in ("train", "valid", "test")}
    with open(tmp_path / "index.pkl", "wb") as f:
        pickle.dump(idx, f)
    ds = DeviceForecastingDataset(str(tmp_path / "data.pkl"), str(tmp_path / "index.pkl"), "valid", L)

    class Runner:
        def __init__(self, model):
            self.model = model

        def to_running_device(self, t):
            return t.cuda()

    model.eval_cache_bytes = _bytes(9)
    model.tsformer._events = []
    st = model.eval_cache_stats

    def iterate(prefetch):
        look = LookaheadLoader(torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False), Runner(model), prefetch=prefetch)
        refs, outs = [], []
        with torch.no_grad():
            for fut, hist, ref in look:
                refs.append(ref)
                outs.append(model(history_data=hist, long_history_data=ref[:, :, :, [0, 1, 2]], future_data=None, batch_seen=0, epoch=1)[2].clone())
        return refs, outs, look

    refs, first, _ = iterate(False)
    assert [r.t0_host for r in refs] == [tuple(b) for b in BATCHES]
    assert all(torch.equal(r.t0.cpu(), torch.tensor(b)) for r, b in zip(refs, BATCHES))
    assert len(model.tsformer._events) == 3 and (st["window_misses"], st["window_hits"]) == (9, 0)
    _, second, _ = iterate(False)
    assert len(model.tsformer._events) == 3 and (st["window_misses"], st["window_hits"]) == (9, 9)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    # announced batches whose windows are all stored queue nothing
    _, third, look = iterate(True)
    assert look.prefetched_batches == 2 and not model._prefetched
    assert len(model.tsformer._events) == 3 and st["window_hits"] == 18
    assert all(torch.equal(x, y) for x, y in zip(first, third))
