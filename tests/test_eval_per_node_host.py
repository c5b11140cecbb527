"""Per-node evaluation metrics, host side: the numpy restatement (tests/eval_nodes_ref.py) against the numbers the reference's own
masked_mae / masked_rmse / masked_mape gave per node (tests/golden/eval_per_node_cases.npz, tools/make_eval_per_node_golden.py), the
table-size arithmetic of the library, and the refusals that need no device.  The device side: tests/test_gpu_eval_per_node.py.

Bound: relative 1e-5 (absolute 1e-6 where the reference gives 0), the bound tests/test_gpu_eval_metrics.py uses against the same float32
reference functions: the reference is an f32 mean over at most 768 elements here, the restatement sums the same f32 terms in f64."""
import numpy as np
import pytest

from tests import eval_nodes_ref as R

CASES = ["a", "b", "h64", "live", "n257", "nan", "one", "pn"]


def assert_close(got, want, rel, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.where(want == 0.0, 1e-6, rel * np.abs(want))
    err = np.abs(got - want)
    print(f"{what}: largest |difference| / bound = {float(np.max(err / bound)):.3e}")
    assert got.shape == want.shape and np.all(err <= bound), (what, got, want)


def test_fixture_holds_the_cases_of_the_issue():
    z = R.load_fixture()
    assert sorted(z["cases"].tolist()) == CASES
    shapes = {name: z[f"{name}.pred"].shape for name in CASES}
    assert shapes == {"a": (7, 12, 5), "b": (7, 12, 5), "n257": (9, 2, 257), "one": (1, 1, 1), "live": (1, 1, 1), "h64": (2, 64, 3),
                      "nan": (7, 12, 5), "pn": (7, 12, 5)}
    assert np.isnan(z["nan.null_val"]) and z["pn.scale"].shape == (5,) and z["b.real"].shape == (7, 12, 5, 3) and int(z["b.channel"]) == 1
    for name in CASES:
        c = R.case_of(z, name)
        B, H, N = c["pred"].shape
        assert c["expected"].shape == (N, H + 1, 3) and c["expected"].dtype == np.float64 and sum(c["split"]) == B
        zero_nodes = [n for n in range(N) if (c["expected"][n] == 0.0).all()]
        assert zero_nodes == ([c["null_node"]] if c["null_node"] >= 0 else []), (name, zero_nodes)
        if name != "nan":          # (under a NaN null_val a 0.0 label is counted and not a MAPE term: MAPE may be 0 by itself)
            assert (np.delete(c["expected"], zero_nodes, axis=0) > 0.0).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_per_node(name):
    c = R.case_of(R.load_fixture(), name)
    label = c["real"][..., c["channel"]]
    table = R.five_sums(c["pred"], label, c["scale"], c["shift"], c["null_val"])
    B, H, N = c["pred"].shape
    assert table.shape == (5, H, N) and table.dtype == np.float64
    assert_close(R.finished(table), c["expected"], 1e-5, f"{name}: restatement against the reference")
    # the sums are additive over a split of the windows (what the accumulator relies on); counts exactly
    at, parts = 0, np.zeros_like(table)
    for n in c["split"]:
        parts += R.five_sums(c["pred"][at:at + n], label[at:at + n], c["scale"], c["shift"], c["null_val"])
        at += n
    assert np.array_equal(parts[[2, 4]], table[[2, 4]]) and np.allclose(parts, table, rtol=1e-12, atol=0.0)


def test_threshold_labels_of_case_a_fall_on_both_sides():
    """the labels one float32 step either side of 5e-5 and 1e-4 change the counts as the rules say (restatement level)"""
    lo, hi = np.float32(5e-5), np.float32(1e-4)
    y = np.array([np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0)), hi,
                  np.nextafter(hi, np.float32(1))], dtype=np.float32).reshape(6, 1, 1)
    counts = [R.five_sums(y[i:i + 1] + np.float32(1.0), y[i:i + 1])[[2, 4], 0, 0].tolist() for i in range(6)]
    assert counts == [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [1.0, 1.0], [1.0, 1.0]]
    z = R.load_fixture()
    a = z["a.real"][..., 0]
    for v in y.ravel():
        assert (a == v).any() and (a == -v).any()


def test_table_size_query_is_a_pure_host_function():
    lib = pytest.importorskip("step_amd._lib").lib()
    assert lib.step_eval_node_table_doubles(12, 307) == 5 * 12 * 307
    assert lib.step_eval_node_table_doubles(1, 1) == 5 and lib.step_eval_node_table_doubles(64, 883) == 5 * 64 * 883
    assert lib.step_eval_node_table_doubles(64, 2 ** 31 - 1) == 5 * 64 * (2 ** 31 - 1)          # (a long: no 32-bit wrap)
    for H, N in ((0, 5), (65, 5), (-1, 5), (12, 0), (12, -3)):
        assert lib.step_eval_node_table_doubles(H, N) == 0
    assert lib.step_abi_version() == 10


def test_node_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL combinations, sizes, strides and an infinite null_val are refused with STEP_ERR_ARG and a message naming the call; the
    pointers are never dereferenced on the host, so made-up non-NULL addresses stand in for device memory"""
    import ctypes
    from step_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)
    good = dict(pred=p, ps=(60, 5, 1), real=p, rs=(60, 5, 1), B=7, H=12, N=5, null=0.0, table=p, out=p)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.step_eval_node_metrics_accumulate(a["pred"], *a["ps"], a["real"], *a["rs"], a["B"], a["H"], a["N"], 1.0, 0.0, a["null"],
                                                   a["table"], a["out"], None)
        return rc, lib.step_last_error().decode()
    for kw, word in ((dict(pred=None), "NULL pred"), (dict(real=None), "NULL pred or real"), (dict(table=None, out=None), "NULL table and NULL out"),
                     (dict(B=0), "positive"), (dict(N=-1), "positive"), (dict(H=65), "exceeds the 64 horizons"), (dict(ps=(60, 0, 1)), "strides"),
                     (dict(rs=(-60, 5, 1)), "strides"), (dict(B=2 ** 20, N=2 ** 11), "exceeds"), (dict(null=float("inf")), "infinite"),
                     (dict(null=float("-inf")), "infinite")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg and "eval_node_metrics_accumulate" in msg, (kw, rc, msg)
    rc = lib.step_eval_node_metrics_accumulate_nodes(p, 60, 5, 1, p, 60, 5, 1, 7, 12, 5, None, p, 0.0, p, p, None)
    assert rc == 1 and "scale_n" in lib.step_last_error().decode()
    for args, word in (((None, 12, 5, p), "NULL"), ((p, 12, 5, None), "NULL"), ((p, 0, 5, p), "H = 0"), ((p, 65, 5, p), "H = 65"), ((p, 12, 0, p), "N = 0")):
        rc = lib.step_eval_node_metrics_finish(*args, None)
        assert rc == 1 and word in lib.step_last_error().decode(), (args, lib.step_last_error())


def test_result_fields_are_appended_with_defaults():
    from step_amd.evaluate import EvalResult
    r = EvalResult(np.zeros((2, 3)), np.zeros(3), np.zeros(3), 4, (0, 1))          # existing positional construction
    assert r.per_node is None and r.per_node_overall is None and r.batches == 4
    import dataclasses
    assert [f.name for f in dataclasses.fields(EvalResult)] == ["per_horizon", "overall", "batch_mean", "batches", "horizons", "per_node",
                                                               "per_node_overall"]


class _Refused(Exception):
    pass


def test_refusals_that_need_no_device(monkeypatch):
    import torch
    from step_amd import evaluate as E

    # update(out=) without nodes: refused by the argument check, in front of any launch (an accumulator object without a device)
    m = object.__new__(E.EvalMetrics)
    m.horizons, m.nodes = 12, None
    monkeypatch.setattr(E, "_view3", lambda t, what: torch.zeros(2, 12, 5))
    m._acc = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError, match="needs an accumulator built with nodes"):
        m.update(None, None, out=torch.zeros(2, 12, 5))
    m.nodes = 7
    with pytest.raises(ValueError, match="5 nodes, the accumulator was built with nodes = 7"):
        m.update(None, None)

    # return_predictions="data" (any truthy value) with a process group, and a value that is none of the three: before anything else
    class _Model:
        eval_noise = "window"

        def parameters(self):
            raise _Refused("reached the device lookup")
    for rp in ("data", True):
        with pytest.raises(ValueError, match="return_predictions is not available for a pass spread over ranks"):
            E.evaluate_pass(_Model(), None, [1, 2], process_group=object(), return_predictions=rp)
    with pytest.raises(_Refused):
        E.evaluate_pass(_Model(), None, [1, 2], process_group=object(), per_node=True)          # per_node is not refused there
    with pytest.raises(ValueError, match="must be False, True or"):
        E.evaluate_pass(_Model(), None, [1, 2], return_predictions="normalised")
    with pytest.raises(ValueError, match="nodes = 0"):
        E.EvalMetrics(12, nodes=0)
