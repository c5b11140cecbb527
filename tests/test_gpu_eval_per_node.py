"""Per-node evaluation metrics on the device: step_eval_node_metrics_* (csrc/eval_nodes.hip) through ``EvalMetrics(nodes=N)``,
``STEP.evaluate(per_node=True, return_predictions="data")`` and ``native_runner(test_per_node=True)``, against the numbers the
reference's own metric functions gave per node (tests/golden/eval_per_node_cases.npz, tools/make_eval_per_node_golden.py) and against the
float64 restatement of tests/eval_nodes_ref.py.  Host side: tests/test_eval_per_node_host.py.

Bounds.
  * Finished table against the fixture: relative 1e-5 (absolute 1e-6 where the reference gives 0), the bound of
    tests/test_gpu_eval_metrics.py against the same float32 reference functions.
  * Five-sum table against the restatement: the counts exactly; S_abs and S_sq relative 1e-12 -- their terms use only +, -, * in float32
    and are bit-equal on both sides, so only the order of at most a few hundred f64 additions differs (n * 2^-53 << 1e-12); S_ape
    relative 2.4e-7 -- one float32 division per term is allowed 2 ulp (2 * 2^-23 = 2.4e-7), and all terms are non-negative, so the bound
    on every term is a bound on the sum.  A sum of no terms is exactly 0 on both sides.
  * Two ways of accumulating the same elements (existing accumulator against the table summed over nodes, one update against a split,
    a spread pass against one process, a cached pass against an uncached one): relative 1e-12, f64 sums of identical f32 terms."""
import functools

import numpy as np
import pytest
import torch

from tests import eval_nodes_ref as R
from tests.test_eval_per_node_host import CASES, assert_close

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    return R.load_fixture()


@functools.lru_cache(maxsize=None)
def _case(name):
    """one case with its device tensors (uploaded once, left unchanged) and the restatement's five sums (computed once)"""
    c = R.case_of(_fixture(), name)
    c["dpred"], c["dreal"] = torch.from_numpy(c["pred"]).cuda(), torch.from_numpy(c["real"]).cuda()
    c["sums"] = R.five_sums(c["pred"], c["real"][..., c["channel"]], c["scale"], c["shift"], c["null_val"])
    return c


def _metrics(c, nodes="N"):
    from step_amd import EvalMetrics
    B, H, N = c["pred"].shape
    rescale = (c["scale"], c["shift"]) if c["scale"].ndim else (float(c["scale"]), float(c["shift"]))
    return EvalMetrics(horizons=H, null_val=c["null_val"], rescale=rescale, nodes=N if nodes == "N" else nodes)


def _feed(m, c, split, **kw):
    at = 0
    for n in split:
        m.update(c["dpred"][at:at + n], c["dreal"][at:at + n, :, :, c["channel"]], **kw)
        at += n
    assert at == c["pred"].shape[0]
    return m.result()


def _table(m):
    return m._table.cpu().numpy().reshape(5, m.horizons, m.nodes).copy()


def _whole(res):
    """EvalResult -> [N, H + 1, 3], the fixture's layout"""
    return np.concatenate([res.per_node, res.per_node_overall[:, None, :]], axis=1)


def _assert_sums(got, want, what, ape=2.4e-7):
    assert got.shape == want.shape and got.dtype == np.float64
    for k, rel in ((0, 1e-12), (1, 1e-12), (3, ape)):
        err, bound = np.abs(got[k] - want[k]), rel * np.abs(want[k])
        print(f"{what}: {R.SUMS[k]} largest |difference| / bound = {float(np.max(err[want[k] != 0] / bound[want[k] != 0], initial=0.0)):.3e}")
        assert np.all(err <= bound), (what, R.SUMS[k], float(err.max()))          # (a sum of no terms: 0 on both sides, bound 0)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4]), (what, "counts")


# ---------------------------------------------------------------------------------------------- (a) the kernel against the reference
@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_reference_per_node(name):
    c = _case(name)
    B, H, N = c["pred"].shape
    for split in ([B], c["split"]):
        m = _metrics(c)
        res = _feed(m, c, split)
        assert res.batches == len(split) and res.per_node.shape == (N, H, 3) and res.per_node_overall.shape == (N, 3)
        assert res.per_node.dtype == np.float64 and res.per_node.flags["C_CONTIGUOUS"]
        assert_close(_whole(res), c["expected"], 1e-5, f"{name}, split {split}: finished table against the reference")
        _assert_sums(_table(m), c["sums"], f"{name}, split {split}: five sums against the restatement")
        # one f64 division and one square root (an ulp each), and for row H the order of at most 64 additions: below 70 * 2^-53 < 2e-14
        assert_close(_whole(res), R.finished(_table(m)), 2e-14, f"{name}: the finish kernel against the restatement's on the same sums")
        if c["null_node"] >= 0:
            assert (_whole(res)[c["null_node"]] == 0.0).all()          # a count of 0 gives exactly 0


# ---------------------------------------------------------------------------------------------- (b) against the existing accumulator
@pytest.mark.parametrize("name", CASES)
def test_table_summed_over_nodes_is_the_existing_accumulator(name):
    c = _case(name)
    B, H, N = c["pred"].shape
    m = _metrics(c)
    res = _feed(m, c, c["split"])
    acc = m._acc.cpu().numpy()[:5 * H].reshape(H, 5).T          # [5, H]
    over_nodes = _table(m).sum(axis=2)
    assert np.array_equal(over_nodes[[2, 4]], acc[[2, 4]])
    for k in (0, 1, 3):
        assert np.all(np.abs(over_nodes[k] - acc[k]) <= 1e-12 * np.abs(acc[k])), (name, R.SUMS[k], over_nodes[k], acc[k])
    # the per-horizon fields are those of an accumulator without nodes
    plain = _feed(_metrics(c, nodes=None), c, c["split"])
    assert plain.per_node is None and plain.per_node_overall is None
    for x, y in ((res.per_horizon, plain.per_horizon), (res.overall, plain.overall), (res.batch_mean, plain.batch_mean)):
        assert_close(x, y, 1e-12, f"{name}: the existing launch next to the per-node one")          # (its atomics' order is not fixed)
    if N == 1:
        assert_close(res.per_node_overall[0], res.overall, 1e-12, f"{name}: one node, per_node_overall against overall")
        assert_close(res.per_node[0], res.per_horizon, 1e-12, f"{name}: one node, per_node against per_horizon")


# ---------------------------------------------------------------------------------------------- (c) the export
def _same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype == torch.float32 and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", ["a", "b", "n257", "nan", "pn"])
def test_export_is_the_rescaled_prediction_bit_for_bit(name):
    c = _case(name)
    B, H, N = c["pred"].shape
    pred, label = c["dpred"], c["dreal"][..., c["channel"]]
    scale, shift = torch.from_numpy(np.asarray(c["scale"])).cuda(), torch.from_numpy(np.asarray(c["shift"])).cuda()
    want = pred * scale + shift          # torch: a rounded multiply, then a rounded add; [N] scalers broadcast along the nodes
    assert torch.isnan(want).any() == bool(np.isnan(c["pred"]).any())
    by_node = pred.transpose(1, 2).contiguous()          # stored [B, N, H]
    view = by_node.transpose(1, 2)
    assert view.shape == pred.shape and (H == 1 or N == 1 or not view.is_contiguous())
    plain = _feed(_metrics(c), c, [B])
    for what, p in (("[B, H, N]", pred), ("[B, H, N, 1]", pred.unsqueeze(-1)), ("a transposed view of [B, N, H]", view)):
        m = _metrics(c)
        out = torch.full((B, H, N), -7.0, device="cuda")
        m.update(p, label, out=out)
        assert _same_bits(out, want), (name, what)
        assert np.array_equal(m.result().per_node, plain.per_node), (name, what)          # the sums do not change with the export
    # split updates write their own windows; a grouped update writes all of them
    for kw, split in ((dict(), c["split"]), (dict(group=c["split"][0]), [B])):
        m = _metrics(c)
        out, at = torch.full((B, H, N), -7.0, device="cuda"), 0
        for n in split:
            m.update(pred[at:at + n], label[at:at + n], out=out[at:at + n], **kw)
            at += n
        assert _same_bits(out, want), (name, kw)
    # the export alone (NULL table) through the C entry point
    import ctypes
    from step_amd import _lib
    out = torch.full((B, H, N), -7.0, device="cuda")
    args = [_lib.ptr(pred), *pred.stride(), ctypes.c_void_p(label.data_ptr()), *label.stride(), B, H, N]
    if c["scale"].ndim:
        _lib.call("step_eval_node_metrics_accumulate_nodes", *args, _lib.ptr(scale), _lib.ptr(shift), c["null_val"], None, _lib.ptr(out), _lib.stream())
    else:
        _lib.call("step_eval_node_metrics_accumulate", *args, float(c["scale"]), float(c["shift"]), c["null_val"], None, _lib.ptr(out), _lib.stream())
    assert _same_bits(out, want)


# ---------------------------------------------------------------------------------------------- (d) reset, result twice, group=, refusals
def test_reset_repeated_result_group_and_refusals():
    c = _case("a")
    B, H, N = c["pred"].shape
    pred, label = c["dpred"], c["dreal"][..., c["channel"]]
    m = _metrics(c)
    assert m._acc.data_ptr() == m._buf.data_ptr() and m._table.data_ptr() == m._buf.data_ptr() + 8 * m._acc.numel()          # ONE allocation
    assert m._buf.numel() == (5 * H + 10) + 5 * H * N
    one = _feed(m, c, [B])
    again = m.result()
    assert np.array_equal(one.per_node, again.per_node) and np.array_equal(one.per_node_overall, again.per_node_overall)
    m.reset()
    assert m.batches == 0 and not m._buf.any()
    parts = _feed(m, c, [3, 3, 1])
    assert_close(_whole(parts), _whole(one), 1e-12, "3 + 3 + 1 windows against one update")
    m.reset()
    m.update(pred, label, group=3)
    grouped = m.result()
    assert grouped.batches == 3 and np.array_equal(grouped.per_node, parts.per_node)          # the same additions in the same order
    assert_close(grouped.batch_mean, parts.batch_mean, 1e-12, "group=3 against 3 + 3 + 1, batch mean")
    assert np.array_equal(grouped.per_node_overall, parts.per_node_overall)
    some = m.result(horizons=[2, 11])
    assert some.per_node.shape == (N, 2, 3) and np.array_equal(some.per_node, grouped.per_node[:, [2, 11]])
    assert np.array_equal(some.per_node_overall, grouped.per_node_overall)          # over ALL horizons, whatever is reported
    # refused before anything is launched; the accumulator and the table are untouched
    before = m._buf.clone()
    with pytest.raises(ValueError, match="4 nodes, the accumulator was built with nodes = 5"):
        m.update(pred[:, :, :4], label[:, :, :4])
    out = torch.zeros(B, H, N, device="cuda")
    for bad in (out[:, :, :4], out[:3], out.double(), out.cpu(), out.transpose(1, 2).contiguous().transpose(1, 2), out.reshape(-1)):
        with pytest.raises(ValueError, match="out must be a contiguous f32"):
            m.update(pred, label, out=bad)
    with pytest.raises(ValueError, match="needs an accumulator built with nodes"):
        _metrics(c, nodes=None).update(pred, label, out=out)
    assert torch.equal(m._buf, before) and m.batches == 3 and not out.any()


# ---------------------------------------------------------------------------------------------- (e) STEP.evaluate
def _host_label(loader, origins):
    series = loader.data[:, :, 0].cpu()
    return torch.stack([series[t:t + 12] for t in origins]).numpy()          # normalised, [W, 12, N]


class _KeptCopies:
    """counts ``Tensor.copy_`` into a device tensor [.., 12, 37] while active: the ``copy_`` per batch of ``return_predictions=True``"""

    def __enter__(self):
        self.count, self._saved = 0, torch.Tensor.copy_

        def counted(t, *args, _original=self._saved, **kwargs):
            if t.is_cuda and t.dim() == 3 and tuple(t.shape[1:]) == (12, 37):
                self.count += 1
            return _original(t, *args, **kwargs)
        torch.Tensor.copy_ = counted
        return self

    def __exit__(self, *exc):
        torch.Tensor.copy_ = self._saved


def test_evaluate_per_node_and_predictions_in_data_units():
    from tests.test_gpu_eval_cache import _reseed
    from tests.test_gpu_eval_metrics import MEAN, STD, _setup
    model, loader, origins = _setup(cache_windows=9)

    def evaluate(**kw):
        _reseed(model)
        with _KeptCopies() as copies:
            out = model.evaluate(loader, origins, scaler=(MEAN, STD), batch_size=4, **kw)
        return out, copies.count
    (plain, normalised), copies = evaluate(return_predictions=True)          # what it returns today: the normalised predictions
    assert plain.per_node is None and plain.per_node_overall is None and copies == 3 and model.eval_cache_stats["windows_stored"] == 9
    (res, data), copies = evaluate(per_node=True, return_predictions="data")
    assert copies == 0                                                        # stored by the kernel: no copy_ per batch
    assert data.shape == (9, 12, 37) and data.is_cuda and _same_bits(data, normalised * STD + MEAN)
    for x, y in ((res.per_horizon, plain.per_horizon), (res.overall, plain.overall), (res.batch_mean, plain.batch_mean)):
        assert_close(x, y, 1e-12, "the per-horizon tables next to the per-node launch")
    assert res.per_node.shape == (37, 12, 3) and res.per_node_overall.shape == (37, 3) and res.batches == 3
    want = R.finished(R.five_sums(normalised.cpu().numpy(), _host_label(loader, origins), STD, MEAN, 0.0))
    got = _whole(res)
    for k, rel in ((0, 1e-12), (1, 1e-12), (2, 2.4e-7)):          # MAE and RMSE from S_abs / S_sq, MAPE from S_ape: the bounds of the sums
        assert_close(got[..., k], want[..., k], rel, f"evaluate per node, column {k}, against the restatement")
    assert (got > 0.0).all()
    # "data" alone implies the node launch; selected horizons select the per-node rows too; a further cached pass gives the same table
    (second, data2), copies = evaluate(return_predictions="data", horizons=[2, 11])
    assert model.eval_cache_stats["window_hits"] == 18 and copies == 0 and _same_bits(data2, data)
    assert second.per_node.shape == (37, 2, 3)
    assert_close(second.per_node, res.per_node[:, [2, 11]], 1e-12, "cached pass, per node")
    assert_close(second.per_node_overall, res.per_node_overall, 1e-12, "cached pass, per node overall")
    # per_node alone: no predictions come back; with the plain switch the normalised ones do
    third, copies = evaluate(per_node=True)
    assert copies == 0
    assert_close(_whole(third), got, 1e-12, "per_node=True alone")
    (_r, kept), copies = evaluate(per_node=True, return_predictions=True)
    assert copies == 3 and torch.equal(kept, normalised)
    with pytest.raises(ValueError, match="must be False, True or"):
        model.evaluate(loader, origins, return_predictions="raw")


def test_the_switches_are_arguments_with_the_defaults_of_the_issue():
    import inspect
    from step_amd import STEP, EvalMetrics
    from step_amd.evaluate import evaluate_pass
    from step_amd.runner import native_runner
    assert inspect.signature(native_runner).parameters["test_per_node"].default is False
    assert inspect.signature(EvalMetrics.__init__).parameters["nodes"].default is None
    assert inspect.signature(EvalMetrics.update).parameters["out"].default is None
    for f in (STEP.evaluate, evaluate_pass):
        assert inspect.signature(f).parameters["per_node"].default is False and inspect.signature(f).parameters["return_predictions"].default is False


# ---------------------------------------------------------------------------------------------- (f) two ranks on one card
def test_per_node_table_of_a_pass_spread_over_two_ranks(tmp_path):
    from tests.two_ranks import run_two_ranks
    run_two_ranks("eval_per_node_worker.py", tmp_path, timeout=300)


# ---------------------------------------------------------------------------------------------- (g) the runner
def test_runner_keeps_the_test_result_and_logs_one_more_line():
    from step_amd.runner import native_runner
    from tests.runner_double import masked_mae
    from tests.spread_double import TestPassDouble
    from tests.test_gpu_eval_cache import BATCHES, _fresh, _reseed
    from tests.test_gpu_eval_metrics import MEAN, STD
    from tests.test_gpu_native_test_pass import LINE, _Readbacks
    from tests.test_gpu_runner_eval import _batches
    model, loader = _fresh("bf16")
    data = _batches(loader)

    def run(**switches):
        runner = native_runner(TestPassDouble, **switches)({"model": model, "loss": masked_mae, "scaler": (MEAN, STD), "cl": None})
        runner.test_data_loader = data
        runner.reset_epoch_meters()
        _reseed(model)
        model.eval()
        with _Readbacks() as rb:
            runner.test()
        return runner, rb.count
    plain, _n = run(native_test=True)
    assert plain.test_result is None and len(plain.logger.lines) == 12 and plain.eval_readbacks == 1
    runner, readbacks = run(native_test=True, test_per_node=True)
    assert runner.eval_readbacks == 1 and readbacks == 1 and runner.test_base_calls == 0          # still ONE read-back for the pass
    assert runner.logger.lines[:12] == plain.logger.lines and all(LINE.match(line) for line in runner.logger.lines[:12])
    assert len(runner.logger.lines) == 13
    assert set(runner.meters) == set(plain.meters)
    for k in ("test_MAE", "test_RMSE", "test_MAPE"):
        assert runner.meters[k].avg == pytest.approx(plain.meters[k].avg, rel=1e-12), k
    res = runner.test_result
    assert res.per_node.shape == (37, 12, 3) and res.per_node_overall.shape == (37, 3)
    _reseed(model)
    want = model.evaluate(loader, [t for b in BATCHES for t in b], scaler=(MEAN, STD), batch_size=3, per_node=True)
    assert_close(res.per_node_overall, want.per_node_overall, 1e-12, "runner per node overall against STEP.evaluate")
    assert_close(res.per_node, want.per_node, 1e-12, "runner per node against STEP.evaluate")
    worst = sorted(range(37), key=lambda n: (-res.per_node_overall[n, 0], n))[:5]
    line = runner.logger.lines[12]
    assert line.endswith(", ".join("{:d}: {:.4f}".format(n, res.per_node_overall[n, 0]) for n in worst)) and "sensor" in line
    # without native_test in effect the switch does nothing, and rank 0 warns once
    with pytest.warns(UserWarning, match="test_per_node needs native_test"):
        base, _n = run(native_test=False, test_per_node=True)
    assert base.test_base_calls == 1 and base.test_result is None and len(base.logger.lines) == 12
