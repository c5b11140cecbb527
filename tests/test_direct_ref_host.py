"""Pin the float64 helper of the direct kernel tests (tests/direct_ref.py) to the reference's own numbers (tests/golden/*.npz).

The direct GPU tests measure the kernels against ``gwnet_ref(float64)`` / ``edges_ref(float64)`` / ``global_ref(float64)``; here those are
fed the golden inputs and must land on the golden outputs, so a mistake in the helper (a transposed prediction, a mis-keyed parameter,
the noise eps added in the wrong precision) cannot pass as a kernel error or hide one.  The bf16 operand model of the global branch
is held to ``global_ref`` with its rounding switched off, and the inputs of every shape of tests/test_gpu_dgl_global_direct.py to the
conditioning its tolerance rule relies on.  No GPU."""
import pytest
import torch

from oracle import step_oracle as O
from tests import direct_ref as D
from tests.helpers import load_golden, params_of, rel_l2, max_abs

PRE = "discrete_graph_learning."


@pytest.fixture(scope="module", params=["step_tiny", "step_small"])
def golden(request):
    """golden inputs, the f32 oracle's step on them (what tests/test_oracle_golden.py pins) and the float64 helper's edge half"""
    g32, g64 = load_golden(request.param), load_golden(request.param, torch.float64)
    N, L, T_train, B, k, epoch, training = [int(x) for x in g32["meta"]]
    aux = {}
    with torch.no_grad():
        pred32, theta32, _, _ = O.step_forward(g32["in.hist"], g32["in.long_hist0"].unsqueeze(-1), g32["in.node_feats"],
                                               params_of(g32, requires_grad=False), g32["in.u"], k, epoch if epoch >= 0 else None,
                                               training=bool(training), aux=aux)
        p64 = params_of(g64, requires_grad=False)
    # the global feature through global_ref's forward (StepDglParams names -> state_dict keys): a mis-keyed parameter there would move
    # theta off the golden below
    gcase = {"series": g64["in.node_feats"].t(), "dg": torch.zeros(N, 100, dtype=torch.float64),
             "p": {k: p64[D.global_key(k)] for k in D.GLOBAL_TRAINABLE + D.GLOBAL_RUNNING}}
    gfeat = D.global_ref(torch.float64, gcase, training=bool(training))["g"]
    ep = {"fc_out_w": p64[PRE + "fc_out.weight"], "fc_out_b": p64[PRE + "fc_out.bias"], "fc_cat_w": p64[PRE + "fc_cat.weight"],
          "fc_cat_b": p64[PRE + "fc_cat.bias"]}
    e64 = D.edges_ref(torch.float64, ep, gfeat, g32["in.u"])
    e32 = D.edges_ref(torch.float32, ep, gfeat, g32["in.u"])
    return {"g32": g32, "g64": g64, "p64": p64, "B": B, "N": N, "training": bool(training), "pred32": pred32, "theta32": theta32,
            "samp32": aux["sampled_adj"], "e64": e64, "e32": e32}


def _sample(a0):
    N = a0.shape[-1]
    return (a0 >= 0).to(torch.float64) * (1 - torch.eye(N, dtype=torch.float64))


def test_edges_ref_reproduces_golden_theta_and_sample(golden):
    g32, e64, e32 = golden["g32"], golden["e64"], golden["e32"]
    # theta: the golden is the reference's float32 output; the f32 oracle is pinned to it at 2e-5 (tests/test_oracle_golden.py) and the
    # float64 helper must be no further away than that oracle
    err64, err32 = max_abs(e64["theta"], g32["out.theta"]), max_abs(golden["theta32"], g32["out.theta"])
    print(f"theta: max-abs to the golden, float64 helper {err64:.3e}, f32 oracle {err32:.3e}")
    assert err64 <= max(err32, 2.0 ** -23)          # (one float32 ulp below 1: the golden itself is rounded to that)
    # the hard Gumbel sample: equal to the oracle's float32 sample on the golden noise (which the golden prediction was computed from),
    # apart from ties -- entries whose float64 margin lies within four times the float32 error of that margin
    want, got = golden["samp32"].double(), _sample(e64["a0"])
    tie = 4 * max_abs(e32["a0"], e64["a0"])
    diff = (want != got)
    print(f"sample: {int(diff.sum())} of {diff.numel()} entries differ, tie width {tie:.3e}, smallest |a0| {float(e64['a0'].abs().min()):.3e}")
    assert bool((e64["a0"].abs()[diff] <= tie).all())
    assert int(diff.reshape(diff.shape[0], -1).sum(1).max()) <= 4
    # ... and the same rule between the helper in the two precisions
    assert bool((e64["a0"].abs()[_sample(e32["a0"].double()) != got] <= tie).all())


def test_gwnet_ref_is_as_close_to_the_golden_prediction_as_the_f32_oracle(golden):
    g32, g64, p64 = golden["g32"], golden["g64"], golden["p64"]
    sd = {k[len("backend."):]: v for k, v in p64.items() if k.startswith("backend.")}
    last = g64["out.hidden"][:, :, -1, :]
    r = D.gwnet_ref(torch.float64, sd, g64["in.hist"], last, _sample(golden["e64"]["a0"]), torch.ones(golden["B"], 12, golden["N"]),
                    training=golden["training"])
    want = g32["out.pred"][..., 0]                      # [B, 12, N]
    e64, e32 = rel_l2(r["pred"], want), rel_l2(golden["pred32"][..., 0], want)
    print(f"pred: rel-L2 to the golden, float64 helper {e64:.3e}, f32 oracle {e32:.3e}")
    assert e32 < 2e-4                                    # the pin of tests/test_oracle_golden.py
    assert e64 <= e32


def test_hop_model_without_rounding_is_the_plain_path():
    c = D.gwnet_case(2, 13, seed=3)
    args = (torch.float64, c["sd"], c["hist"], c["last"], c["adj"], c["dpred"])
    plain, exact, bf16 = D.gwnet_ref(*args), D.gwnet_ref(*args, hop="exact"), D.gwnet_ref(*args, hop="bf16")
    flat = lambda r: {"pred": r["pred"], "dadj": r["dadj"], **r["grads"], **r["running"]}
    a, b, c16 = flat(plain), flat(exact), flat(bf16)
    assert set(a) == set(b) and len(a) > 100
    for k in a:
        assert max_abs(b[k], a[k]) <= 1e-12 * max(1.0, float(a[k].abs().max())), k
    # the model of all of bf16 mode's contractions: the plain path without rounding, further from it than the hops alone with rounding
    every, every16 = flat(D.gwnet_ref(*args, hop="exact_all")), flat(D.gwnet_ref(*args, hop="bf16_all"))
    for k in a:
        assert max_abs(every[k], a[k]) <= 1e-12 * max(1.0, float(a[k].abs().max())), k
    assert rel_l2(c16["pred"], a["pred"]) < rel_l2(every16["pred"], a["pred"]) < 0.25
    assert rel_l2(every16["end2_b"], a["end2_b"]) < 1e-12          # the sum of dpred: no contraction in front of it
    # with rounding on it is a different computation of the same function: bf16 operands cost 2^-9 per product, far above 1e-12 and
    # (the adjacency gradient is a difference of nearly equal terms, 3 % here) far below the values themselves
    assert 1e-4 < rel_l2(c16["pred"], a["pred"]) < 0.25
    assert 1e-4 < rel_l2(c16["dadj"], a["dadj"]) < 0.25
    assert D._RoundedHop is not None and D.O.nconv.__module__ == "oracle.step_oracle"          # the patch is undone


def test_native_key_covers_the_state_dict():
    sd = D.gwnet_state(5, 0)
    keys = {D.native_key(n) for n in D._all_native_names()}
    assert keys <= set(sd)
    assert {k for k in sd if sd[k].is_floating_point() and not k.startswith("residual_convs.")} == keys
    for i in range(8):          # the BatchNorm tensors are off their defaults
        assert float((sd[f"bn.{i}.weight"] - 1).abs().min()) > 0 and float(sd[f"bn.{i}.running_mean"].abs().min()) > 0


# ----------------------------------------------------------------------------------------- the graph learner's global branch
def test_global_model_without_rounding_is_the_plain_path():
    for (N, T), storages in (((13, 40), ("bf16",)), ((13, 160), ("bf16", "f32"))):
        c = D.global_case(N, T, seed=3)
        a = D.flat_global(D.global_ref(torch.float64, c))
        assert len(a) == 19
        for storage in storages:
            b = D.flat_global(D.global_bf16_model(c, rounding=False, storage=storage))
            assert set(a) == set(b)
            for k in a:
                assert tuple(b[k].shape) == tuple(a[k].shape), k
                assert max_abs(b[k], a[k]) <= 1e-12 * max(1.0, float(a[k].abs().max())), (storage, k)
            # with rounding on it is another computation of the same function: bf16 operands cost 2^-9 per product, far above 1e-12 and
            # far below the values themselves
            r = D.flat_global(D.global_bf16_model(c, storage=storage))
            for k in ("g", "fc_w"):
                assert 1e-4 < rel_l2(r[k], a[k]) < 0.25, (storage, k, rel_l2(r[k], a[k]))
        e = D.global_ref(torch.float64, c, training=False)
        m = D.global_bf16_model(c, rounding=False, training=False)
        assert max_abs(m["g"], e["g"]) <= 1e-12 * max(1.0, float(e["g"].abs().max()))
        for k in D.GLOBAL_RUNNING:          # eval mode leaves the statistics alone, in the reference and in the model
            assert torch.equal(e["running"][k], c["p"][k].double()) and torch.equal(m["running"][k], c["p"][k].double()), k


def test_global_case_moves_the_running_statistics_off_their_defaults():
    c = D.global_case(13, 40)
    for k in D.GLOBAL_RUNNING:
        assert float((c["p"][k] - (1.0 if k.endswith("_rv") else 0.0)).abs().min()) > 0, k
    assert set(c["p"]) == set(D.GLOBAL_TRAINABLE + D.GLOBAL_RUNNING)
    assert torch.equal(D.global_case(13, 40)["series"], c["series"]) and not torch.equal(D.global_case(13, 40, seed=1)["series"], c["series"])


@pytest.mark.parametrize("N,T", D.GLOBAL_SHAPES + D.GLOBAL_FORWARD_ONLY)
def test_global_cases_are_well_conditioned(N, T):
    """Conditions on the INPUTS of the direct GPU tests, not measurements of anything: (1) no BatchNorm channel with a batch variance
    below 1e-3 (a dead ReLU channel divides by sqrt(eps)), (2) the float32 oracle within 2e-5 relative L2 of float64 on every compared
    tensor (an ill-conditioned sum would hide a kernel error inside M * e_f32), and with them (3) the bound M * e_f32 + FLOOR of every
    tensor at or below 1e-4, the tightest fixed bound the rule supersedes."""
    stats = {}
    r64, r32 = D.cached_global_ref(N, T, torch.float64), D.cached_global_ref(N, T, torch.float32)
    D.global_ref(torch.float64, D.cached_global_case(N, T), stats_out=stats)
    count = {"bn1": N * (T - 9), "bn2": N * (T - 18), "bn3": N}
    smallest = min(float((var_u * (count[k] - 1) / count[k]).min()) for k, (_, var_u) in stats.items())
    f64, f32 = D.flat_global(r64), D.flat_global(r32)
    forward_only = (N, T) in D.GLOBAL_FORWARD_ONLY
    errs = {k: rel_l2(f32[k], f64[k]) for k in f64 if not (forward_only and k in D.GLOBAL_TRAINABLE)}
    worst = max(errs, key=errs.get)
    print(f"N={N} T={T}: smallest batch variance {smallest:.2e}, largest e_f32 {errs[worst]:.2e} ({worst})")
    assert smallest >= 1e-3
    assert errs[worst] <= 2e-5, (worst, errs[worst])
    assert D.GLOBAL_M * errs[worst] + D.GLOBAL_FLOOR <= 1e-4, (worst, errs[worst])
