"""Gradient accumulation on the device: ``STEP.set_grad_accumulation(k)`` / ``TSFormer.set_grad_accumulation(k)``, the k backwards
``FusedAdamClip`` then takes, and ``step_dgl_edges_backward_acc`` directly.

What is compared: after a group of k micro-batches ``model._flat_grad`` against the FLOAT64 SUM of the k gradients computed one at a
time (``zero_grad()`` -> forward -> backward at k = 1, same weights, inputs and seeds), with ``helpers.rel_l2`` on the whole buffer and
per parameter.  A kernel that stores where it should add leaves one micro-batch's gradient in place of the sum: an error of order 1.

Tolerances.  For every family the rel-L2 spread between repeated k = 1 backwards over identical inputs and seeds was measured on an
MI355X over 30 pairs (``spread_of_repeats`` below; the f32 atomics of the weight-gradient contractions make it non-zero), and the
bound is 4 x the largest value (the project's convention).  The accumulated buffer adds the f32 rounding of k - 1 adds
(<= 2^-24 relative each), which is of the floor's size.

MEASURED on an MI355X, largest of 30 pairs (whole buffer / worst parameter) -> bound = 4 x:
  STEP f32             6.53e-8 / 1.26e-6  ->  2.61e-7 / 5.04e-6     after a group: 5.4e-8 .. 6.0e-8 whole
  STEP bf16            3.05e-4 / 7.80e-3  ->  1.22e-3 / 3.12e-2     after a group: 1.5e-4 .. 2.6e-4 whole, 8.4e-3 worst parameter (bf16
                                                                    operand roundings flip with the order of the atomics upstream)
  pre-training f32     5.32e-8 / 1.67e-7  ->  2.13e-7 / 6.66e-7     after a group: 5.4e-8 .. 6.3e-8 whole, 2.0e-7 worst parameter
  pre-training bf16    6.51e-8 / 1.59e-7  ->  2.61e-7 / 6.37e-7     after a group: 5.7e-8 .. 6.5e-8 whole, 1.9e-7 worst parameter
  edge dg              0 / 0 at all seven shapes: nothing that feeds dg uses atomics, repeated backwards are bit-equal.  4 x 0 cannot be
                       met by any float32 buffer compared with a float64 sum, so test 5 uses what is left of the budget above, the f32
                       rounding of the k - 1 adds: (k - 1) x 2^-24 = 5.96e-8 (edge_bound).  Measured: 3.95e-8 .. 4.12e-8.
  two ranks (tests/dp_grad_accum_worker.py, same bounds): STEP f32 4.9e-8, pre-training f32 4.8e-8 .. 5.2e-8.

Per parameter, a gradient that is zero in exact arithmetic (rounding noise around 0: |g| <= ZERO_GRAD of the buffer's largest
parameter norm) is compared by its absolute size against the same 4 x floor of the buffer's norm instead of relative to itself.
"""
import ctypes
import functools
import random

import pytest
import torch

from oracle import step_oracle as O
from tests import direct_ref as D
from tests import optim_ref as R
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu

# family -> (largest whole-buffer spread, largest per-parameter spread) of 30 pairs of repeated k = 1 backwards (module docstring)
FLOOR = {
    "step_f32": (6.528e-08, 1.259e-06),
    "step_bf16": (3.053e-04, 7.800e-03),
    "pt_f32": (5.325e-08, 1.666e-07),
    "pt_bf16": (6.514e-08, 1.592e-07),
    "edge_dg": (0.000e+00, 0.000e+00),
}
ZERO_GRAD = 1e-6
PAIRS = 30


def bound(family, which=0):
    return 4.0 * FLOOR[family][which]


def edge_bound(k):
    """The edge family's floor is exactly 0: nothing that feeds dg uses atomics, repeated backwards are bit-equal, and 4 x 0 would ask a
    float32 buffer to EQUAL a float64 sum, which no float32 arithmetic can (storing the correctly rounded sum already misses it by up
    to 2^-24 relative).  What remains of the budget is the term the floors of the other families absorb: the f32 rounding of the
    k - 1 adds, <= 2^-24 relative each."""
    return bound("edge_dg") + (k - 1) * 2.0 ** -24


# ================================================================================================ STEP: models, micro-batches, gradients
@functools.lru_cache(maxsize=None)
def step_model(mode):
    from tests.test_gpu_step import build_native
    g = load_golden("step_tiny")
    model = build_native(g)
    model.train()
    model.matmul_precision = mode
    return model, g


@functools.lru_cache(maxsize=None)
def step_batch(j):
    """micro-batch j: the golden batch, perturbed with a seeded generator (j = 0: as it is)"""
    from tests.test_gpu_step import inputs_of
    g = load_golden("step_tiny")
    hist, long_hist, fut = inputs_of(g)
    if j:
        gen = torch.Generator().manual_seed(40 + j)
        hist = hist + 0.2 * torch.randn(hist.shape, generator=gen).cuda()
        long_hist = long_hist.clone()
        long_hist[..., 0] += 0.2 * torch.randn(long_hist.shape[:-1], generator=gen).cuda()
        fut = fut + 0.2 * torch.randn(fut.shape, generator=gen).cuda()
    return hist, long_hist, fut


def step_forward(model, g, j, scale):
    """training forward of micro-batch j with its noise pinned (Gumbel / dropout seeds of the step, dropout seed of the encoder)"""
    mean, std = [float(x) for x in g["meta.scaler"]]
    epoch = int(g["meta"][5])
    hist, long_hist, fut = step_batch(j)
    model._seed_ctr = 100 * (j + 1)
    model.tsformer._seed_counter = 10 * (j + 1)
    pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=epoch)
    return O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef) * scale


def step_single(model, g, j, scale):
    """the gradient of micro-batch j alone, at k = 1"""
    model.zero_grad()
    model.set_grad_accumulation(1)
    step_forward(model, g, j, scale).backward()
    torch.cuda.synchronize()
    out = model._flat_grad.clone()
    model.zero_grad()
    return out


@functools.lru_cache(maxsize=None)
def step_sum64(mode, k):
    """float64 sum of the k single gradients (loss scaled by 1 / k), computed once per (mode, k)"""
    model, g = step_model(mode)
    total = None
    for j in range(k):
        s = step_single(model, g, j, 1.0 / k).double()
        total = s if total is None else total + s
    return total.cpu()


def step_group(model, g, k, interleaved, before_backward=None):
    """a group of k micro-batches: fwd, bwd, fwd, bwd (interleaved) or fwd, fwd, ..., bwd, bwd"""
    model.zero_grad()
    model.set_grad_accumulation(k)
    if interleaved:
        for j in range(k):
            loss = step_forward(model, g, j, 1.0 / k)
            if before_backward is not None:
                before_backward(j)
            loss.backward()
    else:
        losses = [step_forward(model, g, j, 1.0 / k) for j in range(k)]
        for j, loss in enumerate(losses):
            if before_backward is not None:
                before_backward(j)
            loss.backward()
    torch.cuda.synchronize()


def step_items(model):
    lay = model._grad_layout()
    return [(n, lay["items"][n][0], lay["items"][n][1]) for n in lay["order"]]


def pt_items(model):
    from step_amd.optim import flat_items
    return [(n, off, p.numel()) for n, off, p in flat_items(model)]


def held(tag, family, flat, ref64, items):
    """whole buffer and every parameter against the float64 reference; every figure printed before anything is asserted"""
    flat, ref64 = flat.detach().double().cpu(), ref64.double().cpu()
    assert bool(torch.isfinite(flat).all()), tag
    whole = rel_l2(flat, ref64)
    b_whole, b_param = bound(family, 0), bound(family, 1)
    print(f"ACCUM {tag} whole buffer rel_l2={whole:.3e} bound={b_whole:.3e}")
    norms = {n: float(ref64[o:o + c].norm()) for n, o, c in items}
    top, total = max(norms.values()), float(ref64.norm())
    bad = []
    for n, o, c in items:
        a, b = flat[o:o + c], ref64[o:o + c]
        if norms[n] <= ZERO_GRAD * top:
            e, lim, kind = float((a - b).norm()) / total, b_whole, "abs/|buffer|"
        else:
            e, lim, kind = rel_l2(a, b), b_param, "rel_l2"
        if e > 0.25 * lim and len(bad) < 4:
            print(f"ACCUM {tag} {n:<48s} {kind} {e:.3e} bound={lim:.3e}" + ("" if e <= lim else "   <-- ABOVE"))
        if not e <= lim:
            bad.append((n, e, lim))
    assert whole <= b_whole, (tag, whole, b_whole)
    assert not bad, (tag, len(bad), bad[:4])


def spread(a, b, items):
    """(whole-buffer rel_l2, worst per-parameter rel_l2 over the parameters above ZERO_GRAD) between two runs of the same thing"""
    a, b = a.double().cpu(), b.double().cpu()
    norms = {n: float(b[o:o + c].norm()) for n, o, c in items}
    top = max(norms.values())
    per = [rel_l2(a[o:o + c], b[o:o + c]) for n, o, c in items if norms[n] > ZERO_GRAD * top]
    return rel_l2(a, b), max(per)


# ================================================================================================ pre-training: the same pieces
@functools.lru_cache(maxsize=None)
def pt_model(mode):
    from tests.test_gpu_pretrain import _model
    g = load_golden("tsformer_pretrain_tiny")
    model = _model(g, g["in.x"].shape[1])
    model.train()
    model.matmul_precision = mode
    return model, g


@functools.lru_cache(maxsize=None)
def pt_batch(j):
    x = load_golden("tsformer_pretrain_tiny")["in.x"]
    if j:
        x = x + 0.2 * torch.randn(x.shape, generator=torch.Generator().manual_seed(60 + j))
    return x.cuda()


def pt_forward(model, j, p, scale):
    model.dropout_p = p
    model._seed_ctr2 = 20 * (j + 1)
    random.seed(5 + j)          # the token masks
    recon, label = model(history_data=pt_batch(j), future_data=None, batch_seen=0, epoch=1)
    return O.masked_mae(recon * 150.0 + 200.0, label * 150.0 + 200.0, 0.0) * scale


def pt_single(model, j, p, scale):
    model.zero_grad()
    model.set_grad_accumulation(1)
    pt_forward(model, j, p, scale).backward()
    torch.cuda.synchronize()
    out = model._flat_grad.clone()
    model.zero_grad()
    return out


@functools.lru_cache(maxsize=None)
def pt_sum64(mode, k, p):
    model, _ = pt_model(mode)
    total = None
    for j in range(k):
        s = pt_single(model, j, p, 1.0 / k).double()
        total = s if total is None else total + s
    return total.cpu()


def pt_group(model, k, p, interleaved):
    model.zero_grad()
    model.set_grad_accumulation(k)
    if interleaved:
        for j in range(k):
            pt_forward(model, j, p, 1.0 / k).backward()
    else:
        for loss in [pt_forward(model, j, p, 1.0 / k) for j in range(k)]:
            loss.backward()
    torch.cuda.synchronize()


# ================================================================================================ the edge backward, directly
def _incoming(case, i):
    """the incoming gradients (dtheta, dadj) of micro-batch i on the case's forward: seeded, of the case's shapes, unit scale (the case's
    own carry one planted 1e30, which would be the whole norm of the sum)"""
    gen = torch.Generator().manual_seed(1000 * case["N"] + 10 * case["B"] + i)
    return torch.randn(case["dtheta"].shape, generator=gen), torch.randn(case["dadj"].shape, generator=gen)


def run_edges_twice(case, accumulate):
    """one forward, then two backwards with different incoming gradients.  accumulate: both through step_dgl_edges_backward_acc into
    ONE dg (dg_accumulate 0, then 1; dg starts as NaN bytes); else two storing calls of step_dgl_edges_backward into two.  -> dg tensors"""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    dev = torch.device("cuda")
    B, N = case["B"], case["N"]
    lib = L.lib()
    ep = {k: v.to(dev).contiguous() for k, v in case["ep"].items()}
    struct = fill_dgl_struct(ep, 0)
    g = case["g"].to(dev).contiguous()
    u = case["u"].to(dev).contiguous()
    saved = D._nan_floats(lib.step_dgl_edges_saved_floats(B, N), dev)
    to = int(lib.step_dgl_edges_theta_offset(N))
    theta = saved[to:to + B * N * N].view(B, N, N)
    adj = D._nan_floats(B * N * N, dev).view(B, N, N)
    st = L.stream()
    L.call("step_dgl_edges_forward", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(u), 1, D.TEMPERATURE, L.ptr(saved), L.ptr(theta), L.ptr(adj), st)
    grads = {k: torch.zeros_like(v) for k, v in ep.items()}
    gstruct = fill_dgl_struct(grads, 0)
    incoming = [_incoming(case, 0), _incoming(case, 1)]
    out = []
    dg = D._nan_floats(N * 100, dev).view(N, 100)
    for i, (dtheta, dadj) in enumerate(incoming):
        dtheta, dadj = dtheta.to(dev).contiguous(), dadj.to(dev).contiguous()
        work = D._nan_floats(lib.step_dgl_edges_work_floats(N), dev)
        if accumulate:
            L.call("step_dgl_edges_backward_acc", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(saved), L.ptr(dtheta), L.ptr(dadj), D.TEMPERATURE,
                   L.ptr(work), ctypes.byref(gstruct), L.ptr(dg), int(i > 0), None, st)
        else:
            dg = D._nan_floats(N * 100, dev).view(N, 100)
            L.call("step_dgl_edges_backward", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(saved), L.ptr(dtheta), L.ptr(dadj), D.TEMPERATURE,
                   L.ptr(work), ctypes.byref(gstruct), L.ptr(dg), None, st)
            torch.cuda.synchronize()
            out.append(dg.cpu())
    torch.cuda.synchronize()
    return out if not accumulate else [dg.cpu()]


def edge_shapes():
    from tests.test_gpu_dgl_edges_direct import SHAPES
    return SHAPES


# ================================================================================================ the floors (what the bounds come from)
def spread_of_repeats(family, pairs=PAIRS):
    """largest (whole-buffer, per-parameter) rel-L2 spread over `pairs` pairs of repeated k = 1 backwards with identical inputs and
    seeds: run i against run i + 1"""
    worst = [0.0, 0.0]
    if family.startswith("step_"):
        model, g = step_model(family[5:])
        items = step_items(model)
        runs = [step_single(model, g, 0, 1.0).cpu() for _ in range(pairs + 1)]
    elif family.startswith("pt_"):
        model, _ = pt_model(family[3:])
        items = pt_items(model)
        runs = [pt_single(model, 0, 0.1, 1.0).cpu() for _ in range(pairs + 1)]
    else:
        for B, N in edge_shapes():
            c = D.cached_edge_case(B, N)
            runs = [run_edges_twice(c, False)[0].reshape(-1) for _ in range(pairs + 1)]
            for a, b in zip(runs, runs[1:]):
                worst[0] = max(worst[0], rel_l2(a, b))
        return worst[0], worst[0]
    for a, b in zip(runs, runs[1:]):
        w, p = spread(a, b, items)
        worst = [max(worst[0], w), max(worst[1], p)]
    return tuple(worst)


# ================================================================================================ 1. sum, STEP
@pytest.mark.parametrize("interleaved", [True, False], ids=["fbfb", "ffbb"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_step_group_holds_the_sum_of_its_micro_batches(mode, k, interleaved):
    model, g = step_model(mode)
    ref = step_sum64(mode, k)
    step_group(model, g, k, interleaved)
    assert model._backward_count == k
    held(f"STEP {mode} k={k} {'fbfb' if interleaved else 'ffbb'}", "step_" + mode, model._flat_grad, ref, step_items(model))
    model.zero_grad()


# ================================================================================================ 2. the global branch once
def test_global_branch_runs_once_per_group(monkeypatch):
    from step_amd import _lib
    model, g = step_model("f32")
    dgl, be = model.discrete_graph_learning, model.backend
    learner, backbone = (dgl.bn1, dgl.bn2, dgl.bn3), list(be.bn)[:7]
    sd0 = {n: v.clone() for n, v in model.state_dict().items()}
    # one k = 1 forward from the same statistics: what the learner's BatchNorm layers must hold after a whole group
    model.zero_grad()
    model.set_grad_accumulation(1)
    step_forward(model, g, 0, 1.0)
    torch.cuda.synchronize()
    want = {i: (m.running_mean.clone(), m.running_var.clone()) for i, m in enumerate(learner)}
    model.zero_grad()
    model.load_state_dict(sd0)
    counts0 = [int(m.num_batches_tracked) for m in learner + tuple(backbone)]
    events = []
    real = _lib.call

    def recording(name, *args):
        events.append((name, args[8] if name == "step_dgl_global_backward_phase" else None))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)
    step_group(model, g, 3, True, before_backward=lambda j: events.append(("backward", j)))
    monkeypatch.setattr(_lib, "call", real)
    names = [e[0] for e in events]
    assert names.count("step_dgl_global_forward") == 1
    assert names.index("step_dgl_global_forward") < names.index("backward")          # with the group's first forward
    phases = [(i, e[1]) for i, e in enumerate(events) if e[0] == "step_dgl_global_backward_phase"]
    assert [p for _, p in phases] == [1 | 16, 2]          # phase 1 with STEP_DGL_FRESH_FC_GRAD, then phase 2
    third = max(i for i, e in enumerate(events) if e[0] == "backward")
    assert events[third] == ("backward", 2) and all(i > third for i, _ in phases)          # in the third backward
    assert names.count("step_dgl_edges_backward_acc") == 3 and names.count("step_dgl_edges_backward") == 0
    assert names.count("step_gwnet_backward") == 3 and names.count("step_dgl_edges_forward_dyn") == 3
    counts1 = [int(m.num_batches_tracked) for m in learner + tuple(backbone)]
    assert [b - a for a, b in zip(counts0, counts1)] == [1, 1, 1] + [3] * 7
    for i, m in enumerate(learner):
        for name, got, ref in (("running_mean", m.running_mean, want[i][0]), ("running_var", m.running_var, want[i][1])):
            e = rel_l2(got.cpu(), ref.cpu())
            print(f"ACCUM learner bn{i + 1}.{name} after a group of 3 vs one k = 1 forward: rel_l2={e:.3e} bound={bound('step_f32'):.3e}")
            assert e <= bound("step_f32")
    # eval-mode and no_grad forwards neither use nor disturb an open group
    model.zero_grad()
    model.set_grad_accumulation(2)
    loss0 = step_forward(model, g, 0, 0.5)
    grp = model._acc
    kept = grp["kept"]
    with torch.no_grad():
        step_forward(model, g, 1, 0.5)
    model.eval()
    with torch.no_grad():
        step_forward(model, g, 1, 0.5)
    model.train()
    assert model._acc is grp and grp["fwd"] == 1 and grp["kept"] is kept
    loss0.backward()
    step_forward(model, g, 1, 0.5).backward()
    torch.cuda.synchronize()
    held("STEP f32 k=2 with eval / no_grad forwards inside the group", "step_f32", model._flat_grad, step_sum64("f32", 2), step_items(model))
    model.zero_grad()
    model.set_grad_accumulation(1)
    model.load_state_dict(sd0)


# ================================================================================================ 3. the optimizer
@pytest.mark.parametrize("param_grads", [True, False])
def test_fused_optimizer_steps_on_the_sum(param_grads):
    """FusedAdamClip.step() after a group against tests/optim_ref.py's float64 clip + Adam, with the metric of
    tests/test_gpu_optim_direct.py (update, m', v': e_dev <= ADAM_M * e_f32).  The reference is applied to the accumulated buffer as
    the device holds it (float64 of it) -- Adam's first step is sign-like, so the run-to-run noise of a gradient element near zero would
    otherwise be compared, not the optimizer -- and that buffer is held to the float64 sum of the single gradients by the family's bound
    first."""
    from step_amd.optim import FusedAdamClip
    from tests.test_gpu_step import build_native
    g = load_golden("step_tiny")
    model = build_native(g)
    model.train()
    k = 2
    ref_sum = step_sum64("f32", k)          # (same golden weights as the shared model's)
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    max_norm = float(ref_sum.norm()) / 3          # clip factor 1 / 3
    opt = FusedAdamClip(model, weight_decay=1e-5, max_norm=max_norm, param_grads=param_grads, **hp)
    assert model.flat_gradients_only == (not param_grads)
    step_group(model, g, k, True)
    flat_g = model._flat_grad
    held(f"STEP f32 k={k} param_grads={param_grads} before the step", "step_f32", flat_g, ref_sum, step_items(model))
    tr = dict(model._trainable())
    lay = model._grad_layout()
    lo, hi = flat_g.data_ptr(), flat_g.data_ptr() + flat_g.numel() * 4
    for n in lay["order"]:
        if param_grads:
            o, c, _ = lay["items"][n]
            assert tr[n].grad is not None and tr[n].grad.data_ptr() == flat_g.data_ptr() + 4 * o, n          # a view of the buffer
            assert torch.equal(tr[n].grad.reshape(-1), flat_g[o:o + c]), n          # ... that holds the sum
        else:
            assert tr[n].grad is None, n
    p0, g0 = opt.flat.detach().cpu().clone(), flat_g.detach().cpu().clone()
    opt.step()
    torch.cuda.synchronize()
    assert opt.step_count == 1
    kw = {"lr": hp["lr"], "betas": hp["betas"], "eps": hp["eps"], "wd": 1e-5, "max_norm": max_norm}
    kw = {n: R.abi_float(v) for n, v in kw.items()}
    zeros = torch.zeros_like(p0)
    r64 = R.adam_clip_ref(torch.float64, p0, g0, zeros, zeros, step=1, **kw)
    r32 = R.adam_clip_ref(torch.float32, p0, g0, zeros, zeros, step=1, **kw)
    assert float(kw["max_norm"] / (r64[3] + 1e-6)) < 0.5          # the clip is active
    dev = (opt.flat.detach().cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu())
    cmp_ = D.Compare(f"adam after a group, param_grads={param_grads}", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    p64 = p0.double()
    cmp_.add("update", dev[0].double() - p64, r64[0] - p64, r32[0].double() - p64)
    cmp_.add("m", dev[1], r64[1], r32[1])
    cmp_.add("v", dev[2], r64[2], r32[2])
    cmp_.finish()
    assert float(opt.grad_norm) == pytest.approx(float(r64[3]), rel=1e-5)
    # the step ends the group: what it kept is dropped, and a further forward without zero_grad() cannot reuse it
    assert model._acc["kept"] is None
    opt.zero_grad()
    assert model._acc is None and model._flat_grad is None


# ================================================================================================ 4. sum, pre-training
@pytest.mark.parametrize("interleaved", [True, False], ids=["fbfb", "ffbb"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_pretrain_group_holds_the_sum_of_its_micro_batches(mode, p, interleaved):
    model, _ = pt_model(mode)
    k = 2
    ref = pt_sum64(mode, k, p)
    pt_group(model, k, p, interleaved)
    assert model._backward_count == k
    flat = model._flat_grad
    held(f"pre-train {mode} p={p} {'fbfb' if interleaved else 'ffbb'}", "pt_" + mode, flat, ref, pt_items(model))
    for n, off, q in [(n, off, q) for (n, off, c), q in zip(pt_items(model), model._pt_params())]:
        assert q.grad is not None and q.grad.data_ptr() == flat.data_ptr() + 4 * off, n          # .grad aliases the group's buffer
    with pytest.raises(RuntimeError, match="backward 3 of an accumulation group of 2"):
        pt_forward(model, 0, p, 0.5).backward()
    model.zero_grad()
    model.set_grad_accumulation(1)


# ================================================================================================ 5. the edge epilogue, directly
@pytest.mark.parametrize("B,N", edge_shapes())
def test_edge_backward_adds_into_dg(B, N):
    c = D.cached_edge_case(B, N)
    a, b = run_edges_twice(c, False)
    ref = a.double() + b.double()
    (dg,) = run_edges_twice(c, True)
    assert bool(torch.isfinite(dg).all())          # dg started as NaN bytes: the first call stored
    e = rel_l2(dg, ref)
    print(f"ACCUM edges dg B={B} N={N}: rel_l2={e:.3e} bound={edge_bound(2):.3e} (one micro-batch alone: {rel_l2(a, ref):.3e})")
    assert e <= edge_bound(2)


# ================================================================================================ 6. refusals
def test_refusals_and_a_group_discarded_by_zero_grad():
    from step_amd.optim import FusedAdamClip
    from tests.test_gpu_step import build_native
    g = load_golden("step_tiny")
    model = build_native(g)
    model.train()
    opt = FusedAdamClip(model, param_grads=False)
    opt.zero_grad()
    model.set_grad_accumulation(2)
    loss = step_forward(model, g, 0, 0.5)
    with pytest.raises(RuntimeError, match="group is open"):
        model.set_grad_accumulation(3)
    loss.backward()
    with pytest.raises(RuntimeError, match="1 native backwards since zero_grad.., the model accumulates 2 per step"):
        opt.step()          # fewer than k backwards
    # zero_grad() mid-group discards the group cleanly: the next group is correct
    opt.zero_grad()
    assert model._acc is None and model._flat_grad is None and model._backward_count == 0
    step_group(model, g, 2, True)
    held("STEP f32 k=2 after a discarded group", "step_f32", model._flat_grad, step_sum64("f32", 2), step_items(model))
    # a (k + 1)-th backward raises
    extra = step_forward(model, g, 0, 0.5)
    with pytest.raises(RuntimeError, match="backward 3 of an accumulation group of 2"):
        extra.backward()
    # the backward of a forward whose group was closed
    opt.zero_grad()
    stale = step_forward(model, g, 0, 0.5)
    opt.zero_grad()
    with pytest.raises(RuntimeError, match="closed by zero_grad"):
        stale.backward()
    opt.zero_grad()
    # k > 1 with a sharded learner or a GraphedTrainStep
    model.discrete_graph_learning._shard = {"world": 2}
    with pytest.raises(RuntimeError, match="time-sliced graph learner"):
        model.set_grad_accumulation(2)
    model.discrete_graph_learning._shard = None
    model.set_grad_accumulation(1)
    model._dyn = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="GraphedTrainStep"):
        model.set_grad_accumulation(2)
    model._dyn = None
    model.set_grad_accumulation(2)
    from step_amd.graphed import GraphedTrainStep
    with pytest.raises(RuntimeError, match="accumulate 2 micro-batches"):
        GraphedTrainStep(model, opt, step_batch(0))
    # weights rewritten inside a group: the kept pair is dropped, never reused
    opt.zero_grad()
    first = step_forward(model, g, 0, 0.5)
    model.load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError, match="changed inside an accumulation group"):
        step_forward(model, g, 1, 0.5)
    del first
    opt.zero_grad()
    model.set_grad_accumulation(1)
