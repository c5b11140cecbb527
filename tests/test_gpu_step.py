"""End-to-end GPU parity of step_amd.STEP (forward, loss gradient of every trainable tensor, BN running
statistics) against (a) the CPU oracle fed the device encoder's hidden states -- tight tolerances,
everything downstream of the bf16 TSFormer runs in exact-f32 MFMA -- and (b) the reference's own
outputs stored in tests/golden -- loose tolerances that include the bf16 encoder error."""
import numpy as np
import pytest
import torch

from oracle import step_oracle as O
from tests.helpers import load_golden, params_of, rel_l2, max_abs

pytestmark = pytest.mark.gpu


def build_native(g):
    from step_amd import STEP
    N, L, T, B, k, ep, tr = [int(x) for x in g["meta"]]
    targs = dict(patch_size=12, in_channel=1, embed_dim=96, num_heads=4, mlp_ratio=4, dropout=0.1, num_token=L / 12,
                 mask_ratio=0.75, encoder_depth=4, decoder_depth=1, mode="forecasting")
    bargs = dict(num_nodes=N, support_len=2, dropout=0.3, gcn_bool=True, addaptadj=True, aptinit=None, in_dim=2,
                 out_dim=12, residual_channels=32, dilation_channels=32, skip_channels=256, end_channels=512,
                 kernel_size=2, blocks=4, layers=2)
    data = np.zeros((T, N, 3), dtype=np.float32)
    data[:, :, 0] = g["in.node_feats"].numpy()
    m = STEP("SYNTH", None, targs, bargs, dict(dataset_name="SYNTH", k=k, input_seq_len=12, output_seq_len=12,
                                               data=data, train_length=T, tsformer_tokens=L // 12))
    sd = {k_[len("param."):]: v for k_, v in g.items() if k_.startswith("param.")}
    m.load_state_dict(sd, strict=True)           # strict: the reference's state_dict keys/shapes round-trip
    return m.cuda()


def inputs_of(g):
    hist = g["in.hist"].cuda()
    long0 = g["in.long_hist0"]
    long_hist = torch.zeros(*long0.shape, 3)
    long_hist[..., 0] = long0
    return hist, long_hist.cuda(), g["in.future"].cuda()


NAME_MAP = None


def ref_name(k):
    """native tensor name -> reference state_dict key"""
    mod, name = k.split(".", 1)
    if mod == "dgl":
        base, kind = name.rsplit("_", 1)
        return "discrete_graph_learning." + base + (".weight" if kind == "w" else ".bias")
    table = {"nodevec1": "nodevec1", "nodevec2": "nodevec2", "start_w": "start_conv.weight", "start_b": "start_conv.bias",
             "fc_his0_w": "fc_his.0.weight", "fc_his0_b": "fc_his.0.bias", "fc_his2_w": "fc_his.2.weight",
             "fc_his2_b": "fc_his.2.bias", "end1_w": "end_conv_1.weight", "end1_b": "end_conv_1.bias",
             "end2_w": "end_conv_2.weight", "end2_b": "end_conv_2.bias"}
    if name in table:
        return "backend." + table[name]
    stem, idx = name.split(".")
    base, kind = stem.rsplit("_", 1)
    kind = "weight" if kind == "w" else "bias"
    mods = {"filter": "filter_convs", "gate": "gate_convs", "skip": "skip_convs", "bn": "bn", "gconv": "gconv"}
    if base == "gconv":
        return f"backend.gconv.{idx}.mlp.mlp.{kind}"
    return f"backend.{mods[base]}.{idx}.{kind}"


@pytest.mark.parametrize("name", ["step_tiny", "step_small"])
def test_step_training_step_parity(name):
    g = load_golden(name)
    N, L, T, B, k, epoch, tr = [int(x) for x in g["meta"]]
    mean, std = [float(x) for x in g["meta.scaler"]]
    model = build_native(g)
    model.train()
    model.backend.dropout = 0.0
    model.tsformer.dropout_p = 0.0
    model.track_dead_bn7 = name == "step_small"          # one golden with, one without the reference's dead bn.7 statistics
    model._noise_override = g["in.u"]
    hist, long_hist, fut = inputs_of(g)
    pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=epoch)
    assert pred.shape == (B, 12, N, 1) and theta.shape == (B, N, N) and knn.shape == (B, N, N)
    assert coef == pytest.approx(float(g["meta.coef"]))
    loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef)
    loss.backward()
    torch.cuda.synchronize()

    # ---------------- (a) oracle fed the device encoder's hidden states
    P = L // 12
    hid = model._last["hidden_bf16"].float().cpu().view(B, N, P, 96)
    p = params_of(g)
    aux, stats = {}, {}
    o_pred, o_theta, o_knn, o_coef = O.step_forward(g["in.hist"], g["in.long_hist0"].unsqueeze(-1), g["in.node_feats"], p, g["in.u"],
                                                    k, epoch, training=True, stats=stats, hidden=hid,
                                                    hidden_last=model._last["hidden_last"].cpu().view(B, N, 96), aux=aux)
    o_loss = O.step_loss(O.rescale(o_pred, mean, std), O.rescale(g["in.future"][..., [0]], mean, std), o_theta, o_knn, o_coef)
    o_loss.backward()
    assert torch.equal(model._last["sampled_adj"].cpu(), aux["sampled_adj"]), "Gumbel hard sample differs"
    assert max_abs(theta.detach().cpu(), o_theta) < 1e-5
    dk = (knn.cpu() != o_knn).sum().item()
    print(name, "knn entries differing from oracle(native hidden):", dk)
    assert dk <= 2 * B
    e_pred = rel_l2(pred.detach().cpu(), o_pred)
    print(name, "pred rel-L2 vs oracle(native hidden)", e_pred, "loss", float(loss), float(o_loss))
    assert e_pred < 2e-3
    assert float(loss) == pytest.approx(float(o_loss), rel=2e-3)
    worst = 0.0
    errs = {}
    native = dict(model._trainable())
    for kname, t in native.items():
        rk = ref_name(kname)
        og = p[rk].grad
        assert og is not None, rk
        ng = t.grad
        assert ng is not None, kname
        if float(og.abs().max()) < 1e-4:
            assert max_abs(ng.cpu(), og) < 2e-4, kname
            continue
        e = rel_l2(ng.cpu(), og)
        errs[kname] = e
        worst = max(worst, e)
    print(name, "grad rel-L2 vs oracle(native hidden):", {k_: round(v_, 5) for k_, v_ in sorted(errs.items(), key=lambda kv: -kv[1])[:12]})
    bad = {k_: v_ for k_, v_ in errs.items() if v_ > 1e-2}
    assert not bad, bad
    print(name, "worst grad rel-L2 vs oracle(native hidden)", worst)
    # tensors the reference leaves without a gradient stay without one
    for n_, prm in model.named_parameters():
        if n_ in set(str(s) for s in g["meta.nograd"]):
            assert prm.grad is None, n_
    # running statistics (bn.7 is dead code in the reference forward -> not updated here)
    sd = model.state_dict()
    for kk, v in g.items():
        if kk.startswith("after.") and ("bn.7" not in kk or model.track_dead_bn7):
            key = kk[len("after."):]
            if key.endswith("num_batches_tracked"):
                assert int(sd[key]) == int(v), key
            else:
                assert rel_l2(sd[key].cpu(), v) < 2e-3, key

    # ---------------- (b) the reference's own numbers (bf16 encoder error included)
    e_ref = rel_l2(pred.detach().cpu(), g["out.pred"])
    print(name, "pred rel-L2 vs reference", e_ref, "loss vs reference", float(loss), float(g["out.loss"]))
    assert e_ref < 5e-3                          # measured 1.3 .. 1.5e-3 with the default float16 encoder operands
    assert max_abs(theta.detach().cpu(), g["out.theta"]) < 1e-4
    assert float(loss) == pytest.approx(float(g["out.loss"]), rel=1e-3)      # measured 2e-5
    # per-tensor errors are dominated by sign flips of the L1 loss where pred ~ label, so the pass/fail
    # criterion is on the concatenated gradient vector; the worst tensor is reported
    worst, num, den, wname = 0.0, 0.0, 0.0, None
    for kname, t in native.items():
        rg = g.get("grad." + ref_name(kname))
        if rg is None:
            continue
        d = (t.grad.cpu().double() - rg.double())
        num += float((d * d).sum())
        den += float((rg.double() ** 2).sum())
        if float(rg.abs().max()) >= 1e-4:
            e = rel_l2(t.grad.cpu(), rg)
            if e > worst:
                worst, wname = e, kname
    total = (num / den) ** 0.5
    print(name, "whole-gradient rel-L2 vs reference", total, "worst tensor", wname, worst)
    assert total < 0.1


def test_step_eval_mode_matches_reference():
    g = load_golden("step_tiny_eval")
    mean, std = [float(x) for x in g["meta.scaler"]]
    model = build_native(g)
    model.eval()
    model._noise_override = g["in.u"]
    hist, long_hist, fut = inputs_of(g)
    with torch.no_grad():
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=None)
    assert coef == 0
    assert rel_l2(pred.cpu(), g["out.pred"]) < 3e-2
    assert max_abs(theta.cpu(), g["out.theta"]) < 1e-4
    assert (knn.cpu() != g["out.knn"]).sum().item() <= 4
    # running stats untouched in eval
    for kk, v in g.items():
        if kk.startswith("param.") and "running_" in kk:
            assert torch.equal(model.state_dict()[kk[len("param."):]].cpu(), v)


@pytest.mark.parametrize("operand,tol", [("bf16", 3e-2), ("f16", 6e-3)])
def test_step_eval_mode_encoder_operand(operand, tol):
    """The encoder's 16-bit operand type: float16 fragments bring the prediction error vs the reference's own output
    (whose TSFormer is fp32) down by the factor the CPU emulation predicts (tools/encoder_precision_study.py)."""
    g = load_golden("step_tiny_eval")
    model = build_native(g)
    model.eval()
    model.tsformer.encoder_operand = operand
    model._noise_override = g["in.u"]
    hist, long_hist, fut = inputs_of(g)
    with torch.no_grad():
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=None)
    e = rel_l2(pred.cpu(), g["out.pred"])
    print(operand, "pred rel-L2 vs reference", e)
    assert e < tol
    assert (knn.cpu() != g["out.knn"]).sum().item() <= 4


def test_step_device_noise_and_dropout_run():
    """Perf-mode path: on-device Philox Gumbel noise + dropout in TSFormer and gcn."""
    g = load_golden("step_tiny")
    model = build_native(g)
    model.train()
    hist, long_hist, fut = inputs_of(g)
    out = []
    for _ in range(2):
        torch.manual_seed(123)
        model._seed_ctr = 0
        model.tsformer._seed_counter = 0
        model.zero_grad()
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=1)
        loss = O.step_loss(O.rescale(pred[..., [0]], 200.0, 150.0), O.rescale(fut[..., [0]], 200.0, 150.0), theta, knn, coef)
        loss.backward()
        assert torch.isfinite(loss)
        out.append((pred.detach().clone(), model._last["sampled_adj"].clone()))
    dens = float(out[0][1].mean())
    print("sampled adjacency density", dens)
    assert 0.2 < dens < 0.8
    assert torch.equal(out[0][1], out[1][1])          # same seed -> same graph sample
    assert rel_l2(out[0][0].cpu(), out[1][0].cpu()) < 1e-4


def test_fused_adam_clip_matches_torch():
    """step_adam_clip == torch.nn.utils.clip_grad_norm_ + torch.optim.Adam over several steps, and the flattened
    parameters keep driving the native forward.  Both optimizers are fed the same gradients every step (a shadow copy of
    the parameters carries the torch optimizer): two independent training runs would not be comparable, the split-K /
    bias-column reductions use atomics and Adam turns round-off on near-zero gradients into +-lr steps."""
    from step_amd.optim import FusedAdamClip
    g = load_golden("step_tiny")
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs_of(g)
    torch.manual_seed(0)
    model = build_native(g)
    model.train()
    model.backend.dropout = 0.0
    model.tsformer.dropout_p = 0.0
    model._noise_override = g["in.u"]
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    shadow = [p.detach().clone().requires_grad_(True) for _, p in named]
    opt = FusedAdamClip(model, lr=2e-3, weight_decay=1e-5, eps=1e-8, max_norm=3.0)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]        # flattening re-creates the storage
    topt = torch.optim.Adam(shadow, lr=2e-3, weight_decay=1e-5, eps=1e-8)
    losses = []
    for it in range(4):
        opt.zero_grad(set_to_none=True)
        topt.zero_grad(set_to_none=True)
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=it, epoch=1)
        loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef)
        loss.backward()
        for sp, (_, p) in zip(shadow, named):
            sp.grad = None if p.grad is None else p.grad.detach().clone()
        torch.nn.utils.clip_grad_norm_([sp for sp in shadow if sp.grad is not None], max_norm=3.0)
        topt.step()
        opt.step()
        losses.append(float(loss))
        for sp, (n, p) in zip(shadow, named):
            assert max_abs(p.detach().cpu(), sp.detach().cpu()) < 2e-6 + 2e-5 * float(sp.abs().max()), (it, n)
    print("losses", losses)
    assert losses[-1] < losses[0]               # the flattened parameters are the ones the native forward reads
    # a torch Optimizer: the reference's scheduler (CFG.TRAIN.LR_SCHEDULER = MultiStepLR, STEP_PEMS04.py:98-102) drives its learning rate
    assert isinstance(opt, torch.optim.Optimizer)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1, 2], gamma=0.5)
    sched.step(); sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(2e-3 * 0.25)
    sd = opt.state_dict()
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == pytest.approx(2e-3 * 0.25) and opt.step_count == 4
    # one backward per step(): the flat gradient buffer holds the last backward only (gradient accumulation must use torch's Adam)
    opt.zero_grad(set_to_none=True)
    for _ in range(2):
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=9, epoch=1)
        O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef).backward()
    with pytest.raises(RuntimeError, match="2 native backwards"):
        opt.step()
    opt.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match="no native backward"):
        opt.step()


def _opt_setup(param_grads, seed=0):
    from step_amd.optim import FusedAdamClip
    g = load_golden("step_tiny")
    torch.manual_seed(seed)
    model = build_native(g)
    model.train()
    model.backend.dropout = 0.0
    model.tsformer.dropout_p = 0.0
    model._noise_override = g["in.u"]
    return g, model, FusedAdamClip(model, lr=2e-3, weight_decay=1e-5, eps=1e-8, max_norm=3.0, param_grads=param_grads)


def _opt_steps(g, model, opt, n, check=None):
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs_of(g)
    losses = []
    for it in range(n):
        opt.zero_grad(set_to_none=True)
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=it, epoch=1)
        loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef)
        loss.backward()
        if check is not None:
            check(it)
        opt.step()
        losses.append(float(loss))
    return losses


def test_param_grads_alias_flat_buffer_every_step():
    """every .grad must be a VIEW of model._flat_grad on every step (autograd clones a returned view that has another
    owner -- a cached tuple of views did that from the second step on: 105 MB of copies per step, and a DistributedDataParallel wrap
    would have reduced the clones while FusedAdamClip stepped on the unreduced flat buffer)."""
    g, model, opt = _opt_setup(param_grads=True)

    def check(it):
        flat = model._flat_grad
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
        lay = model._grad_layout()
        for (k, p) in model._trainable():
            assert p.grad is not None and lo <= p.grad.data_ptr() < hi, (it, k)
            assert p.grad.data_ptr() == lo + 4 * lay["items"][k][0], (it, k)
    _opt_steps(g, model, opt, 3, check)
    # a cloned gradient is refused instead of silently ignored
    opt.zero_grad(set_to_none=True)
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs_of(g)
    pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=1)
    O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef).backward()
    for p in model._trainable_list():
        p.grad = p.grad.clone()
    with pytest.raises(RuntimeError, match="not a view of the native flat gradient buffer"):
        opt.step()


def test_flat_gradients_only_matches_param_grads():
    """FusedAdamClip(param_grads=False) -- the path bench.py times -- takes the same steps as param_grads=True (which the torch comparison
    above covers): same losses, same parameters, and no .grad is materialised."""
    ga, ma, oa = _opt_setup(param_grads=True)
    gb, mb, ob = _opt_setup(param_grads=False)
    la = _opt_steps(ga, ma, oa, 4)
    lb = _opt_steps(gb, mb, ob, 4, check=lambda it: [None for p in mb._trainable_list() if p.grad is not None and pytest.fail("a .grad exists")])
    assert mb.flat_gradients_only and not ma.flat_gradients_only
    print("param_grads True / False losses", la, lb)
    for a, b in zip(la, lb):
        assert a == pytest.approx(b, rel=2e-5)
    # (two independent runs: split-K / bias-column reductions use atomics and Adam turns round-off on near-zero gradients into +-lr steps,
    #  see test_fused_adam_clip_matches_torch -- so single elements may sit a few lr apart, the parameter vector as a whole may not)
    num = sum(float((pa.detach().double() - pb.detach().double()).pow(2).sum()) for (_, pa), (_, pb) in zip(ma._trainable(), mb._trainable()))
    den = sum(float(pa.detach().double().pow(2).sum()) for _, pa in ma._trainable())
    assert (num / den) ** 0.5 < 1e-3, (num / den) ** 0.5
    for (k, pa), (_, pb) in zip(ma._trainable(), mb._trainable()):
        assert max_abs(pa.detach().cpu(), pb.detach().cpu()) <= 4 * 2e-3 + 1e-6, k
    assert la[-1] < la[0]


def test_native_step_loss_matches_reference_loss():
    """The fused loss kernel (value + both gradients) against the ORACLE's step_loss (oracle/step_oracle.py, pinned to the
    reference's step_loss / masked_mae by tests/test_oracle_golden.py), evaluated on the CPU."""
    from step_amd.step_loss import step_loss_native
    g = torch.Generator().manual_seed(5)
    B, N = 3, 23
    pred = (torch.randn(B, 12, N, 1, generator=g) * 150 + 200).cuda().requires_grad_(True)
    real = (torch.randn(B, 12, N, 1, generator=g) * 150 + 200)
    real[0, :, 3] = 0.0                                         # null values are masked out
    real = real.cuda()
    theta = torch.rand(B, N, N, generator=g).clamp(1e-4, 1 - 1e-4).cuda().requires_grad_(True)
    prior = (torch.rand(B, N, N, generator=g) < 0.1).float().cuda()
    pred_c = pred.detach().cpu().requires_grad_(True)
    theta_c = theta.detach().cpu().requires_grad_(True)
    for coef in (1.0, 0.5, 0):
        l_ref = O.step_loss(pred_c, real.cpu(), theta_c, prior.cpu(), coef, null_val=0.0)
        gp, gt = torch.autograd.grad(l_ref, [pred_c, theta_c], allow_unused=True)
        l_nat = step_loss_native(pred, real, theta, prior, coef, null_val=0.0)
        np_, nt_ = torch.autograd.grad(l_nat * 2.0, [pred, theta], allow_unused=True)
        assert float(l_nat) == pytest.approx(float(l_ref), rel=1e-5)
        assert rel_l2(np_.cpu() / 2.0, gp) < 1e-5
        if coef:
            assert rel_l2(nt_.cpu() / 2.0, gt) < 1e-5
        else:
            assert float(nt_.abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_wavenet_phase_5_plus_6_is_phase_1(mode):
    """step_gwnet_forward_phase: the adjacency-independent start of the WaveNet (phase 5, on a third stream next to the graph learner) +
    the rest (phase 6) give bit-identical predictions, edge probabilities and gradients to the single layer phase (1)."""
    g = load_golden("step_small")
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs_of(g)
    outs = []
    for split in (False, True):
        torch.manual_seed(0)
        model = build_native(g)
        model.train()
        model.matmul_precision = mode
        model.backend.dropout = 0.0
        model.tsformer.dropout_p = 0.0
        model._noise_override = g["in.u"]
        model.split_wavenet_prep = split
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=1)
        O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef).backward()
        torch.cuda.synchronize()
        outs.append((pred.detach().clone(), theta.detach().clone(), {k: v.grad.detach().clone() for k, v in model._trainable() if v.grad is not None}))
    if mode == "bf16":          # (f32 mode: the graph learner's fc product adds its split-K pieces with atomics -- two runs differ in the last bits anyway)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert rel_l2(outs[1][0].cpu(), outs[0][0].cpu()) < 1e-5 and max_abs(outs[1][1].cpu(), outs[0][1].cpu()) < 1e-6
    for k, a in outs[0][2].items():
        if k.startswith("be.") and ("gate" in k or "filter" in k or "skip" in k or "gconv" in k or "bn" in k):
            continue          # (weight gradients of split-K / atomic reductions: equal up to the order of the atomics)
        assert rel_l2(outs[1][2][k].cpu(), a.cpu()) < 1e-5, k


def test_native_masked_metrics_match_the_reference_definitions():
    """step_masked_metrics: MAE / RMSE / MAPE of basicts/metrics/{mae,rmse,mape}.py (restated line by line in tests/optim_ref.py) from
    one launch, including null values, labels below 1e-4 (MAPE zeroes and masks them), a strided label view and an all-masked batch."""
    from step_amd.step_loss import masked_metrics_native
    from tests.optim_ref import masked_metrics_ref as ref
    gen = torch.Generator().manual_seed(3)
    for shape, null in (((8, 12, 307, 1), 0.0), ((3, 12, 37, 1), 0.0), ((2, 12, 20, 1), -1.0)):
        y3 = torch.randn(*shape[:3], 3, generator=gen) * 50 + 100
        y3[..., 0][torch.rand(shape[:3], generator=gen) < 0.2] = null
        y3[..., 0][torch.rand(shape[:3], generator=gen) < 0.05] = 3e-5
        p = y3[..., :1] + torch.randn(*shape, generator=gen) * 10
        want = ref(p, y3[..., :1].contiguous(), null)
        got = masked_metrics_native(p.cuda(), y3.cuda()[..., :1], null).cpu()          # labels: a strided view of the batch tensor
        again = masked_metrics_native(p.cuda(), y3.cuda()[..., :1].contiguous(), null).cpu()          # (the work buffer was left clean)
        print("metrics", shape, null, got.tolist(), want.tolist())
        assert torch.allclose(got, want, rtol=2e-5, atol=1e-6) and torch.equal(got, again)
    y = torch.zeros(2, 12, 5, 1)
    assert masked_metrics_native(torch.ones(2, 12, 5, 1).cuda(), y.cuda(), 0.0).cpu().tolist() == [0.0, 0.0, 0.0]


def test_native_step_loss_with_inverse_scaling_inside():
    """step_loss_native(..., rescale=(mean, std)): the runner's inverse scaling (base_tsf_runner.py:240-250) folded into the loss
    kernels, the target read in place as feature 0 of the [B, 12, N, C] batch tensor -- against the oracle's step_loss on the rescaled
    tensors (value, gradient w.r.t. the NORMALISED prediction, gradient w.r.t. theta); also through retain_graph (the backward
    must not scale its saved gradients in place)."""
    from step_amd.step_loss import step_loss_native, _flat_stride
    g = torch.Generator().manual_seed(6)
    B, N, C = 3, 23, 3
    mean, std = 200.0, 150.0
    pred = torch.randn(B, 12, N, 1, generator=g).cuda().requires_grad_(True)
    fut = torch.randn(B, 12, N, C, generator=g)
    fut[0, :, 3, 0] = -mean / std                                # rescales to the null value 0
    fut = fut.cuda()
    theta = torch.rand(B, N, N, generator=g).clamp(1e-4, 1 - 1e-4).cuda().requires_grad_(True)
    prior = (torch.rand(B, N, N, generator=g) < 0.1).float().cuda()
    assert _flat_stride(fut[..., :1]) == C and _flat_stride(fut) == 1 and _flat_stride(fut[:, :, ::2, :1]) is None
    pred_c = pred.detach().cpu().requires_grad_(True)
    theta_c = theta.detach().cpu().requires_grad_(True)
    l_ref = O.step_loss(O.rescale(pred_c, mean, std), O.rescale(fut.cpu()[..., :1], mean, std), theta_c, prior.cpu(), 0.7, null_val=0.0)
    gp, gt = torch.autograd.grad(l_ref, [pred_c, theta_c])
    for target in (fut[..., :1], fut[..., :1].contiguous(), fut[:, :, :, [0]]):
        l_nat = step_loss_native(pred, target, theta, prior, 0.7, null_val=0.0, rescale=(mean, std))
        a1 = torch.autograd.grad(l_nat * 3.0, [pred, theta], retain_graph=True)
        a2 = torch.autograd.grad(l_nat * 3.0, [pred, theta])
        assert float(l_nat) == pytest.approx(float(l_ref), rel=1e-5)
        for a in (a1, a2):
            assert rel_l2(a[0].cpu() / 3.0, gp) < 1e-5 and rel_l2(a[1].cpu() / 3.0, gt) < 1e-5
    n_null = int((O.rescale(fut.cpu()[..., :1], mean, std).abs() <= 5e-5).sum())
    assert n_null == 12 and float((a2[0][0, :, 3] != 0).sum()) == 0           # the masked targets carry no gradient


@pytest.mark.parametrize("name", ["step_tiny", "step_small"])
def test_step_bf16_matmul_mode(name):
    """matmul_precision="bf16": diffusion hops, their adjoints and the DGL fc on the bf16 matrix cores.  Operand rounding
    is 2^-9 relative per element with random sign, so whole-tensor errors stay at the 1e-3..1e-2 level; the discrete outputs
    (Gumbel sample, kNN prior) must not move."""
    g = load_golden(name)
    N, L, T, B, k, epoch, tr = [int(x) for x in g["meta"]]
    mean, std = [float(x) for x in g["meta.scaler"]]
    outs = {}
    for mode in ("f32", "bf16"):
        model = build_native(g)
        model.train()
        model.matmul_precision = mode
        model.backend.dropout = 0.0
        model.tsformer.dropout_p = 0.0
        model._noise_override = g["in.u"]
        hist, long_hist, fut = inputs_of(g)
        pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=epoch)
        loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef)
        loss.backward()
        torch.cuda.synchronize()
        outs[mode] = dict(pred=pred.detach().cpu(), theta=theta.detach().cpu(), knn=knn.cpu(), loss=float(loss),
                          adj=model._last["sampled_adj"].cpu(), grads={kk: t.grad.cpu() for kk, t in dict(model._trainable()).items()})
    a, b = outs["f32"], outs["bf16"]
    # the prior is a function of the encoder output only; the Gram kernel's split-K atomics can move entries that tie at the
    # k-th similarity
    assert (a["knn"] != b["knn"]).sum().item() <= 2 * B
    flips = (a["adj"] != b["adj"]).sum().item()
    print(name, "Gumbel sample flips f32 -> bf16 fc:", flips, "of", a["adj"].numel())
    assert flips <= max(2, a["adj"].numel() // 500)
    e_pred = rel_l2(b["pred"], a["pred"])
    print(name, "bf16-mode pred rel-L2 vs f32 mode", e_pred, "loss", b["loss"], a["loss"])
    assert e_pred < 2e-2          # 5e-3 .. 1.1e-2 measured (bf16 operands everywhere + bf16 storage of the DGL conv activations)
    assert max_abs(b["theta"], a["theta"]) < 5e-3
    assert b["loss"] == pytest.approx(a["loss"], rel=5e-3)
    if flips == 0:
        num = sum(float(((b["grads"][kk] - a["grads"][kk]) ** 2).sum()) for kk in a["grads"])
        den = sum(float((a["grads"][kk] ** 2).sum()) for kk in a["grads"])
        e_g = (num / den) ** 0.5
        print(name, "bf16-mode whole-gradient rel-L2 vs f32 mode", e_g)
        assert e_g < 5e-2
    e_ref = rel_l2(b["pred"], g["out.pred"])
    print(name, "bf16-mode pred rel-L2 vs reference", e_ref)
    assert e_ref < 4e-2


def test_device_window_loader_matches_tensor_inputs():
    """Index-only loader: gathering the windows on the device gives the same history / future tensors as
    slicing, and STEP.forward on a LongHistoryRef equals the forward on the materialised [B, L, N, C] tensor;
    forecast origins before L rows exist produce the zero history of the reference's dataset."""
    from step_amd import DeviceWindowLoader
    g = load_golden("step_small")
    N, L, T, B, k, epoch, tr = [int(x) for x in g["meta"]]
    gen = torch.Generator().manual_seed(3)
    Tall = L + 200
    data = torch.randn(Tall, N, 3, generator=gen).cuda()
    loader = DeviceWindowLoader(data, L)
    t0 = [L, L + 57, L + 188, L - 5]
    hist, ref, fut = loader.batch(t0)
    for i, t in enumerate(t0):
        assert torch.equal(hist[i], data[t - 12:t])
        assert torch.equal(fut[i], data[t:t + 12])
    long_hist = torch.stack([data[t - L:t] if t >= L else torch.zeros(L, N, 3, device="cuda") for t in t0])
    model = build_native(g)
    model.eval()
    model._noise_override = torch.rand(len(t0), N * N, 2, generator=gen)
    with torch.no_grad():
        a = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=1)
        b = model(history_data=hist, long_history_data=ref, future_data=None, batch_seen=0, epoch=1)
    # same arithmetic on the same encoder input; the DGL fc accumulates its split-K partials with atomics, so two forwards
    # agree to round-off, not bitwise
    assert max_abs(a[1], b[1]) < 1e-5 and rel_l2(a[0].cpu(), b[0].cpu()) < 1e-4
    # kNN prior: threshold ties only (split-K atomics in the Gram).  The zero-history window is all ties (every cosine is 1,
    # SURVEY appendix A.3), so only its number of selected edges is compared.
    assert (a[2][:3] != b[2][:3]).sum().item() <= 6
    assert abs(float(a[2][3].sum() - b[2][3].sum())) <= N


@pytest.mark.parametrize("name", ["step_tiny", "step_small"])
def test_step_training_parity_with_gcn_dropout_masks(name):
    """F.dropout(0.3) after every gcn (graphwavenet/model.py:47): the native forward keeps its keep-masks (already scaled by
    1/0.7) for the backward; the test reads them back (step_gwnet_saved_offset item 0) and the oracle replays the same
    realisation -- prediction, loss and every gradient of the dropout-on training step must agree like the dropout-off ones."""
    import step_amd._lib as L
    g = load_golden(name)
    N, Lh, T, B, k, epoch, tr = [int(x) for x in g["meta"]]
    mean, std = [float(x) for x in g["meta.scaler"]]
    model = build_native(g)
    model.train()
    model.tsformer.dropout_p = 0.0            # the encoder's dropout has its own mask-exact test (test_gpu_kernels.py)
    assert model.backend.dropout == pytest.approx(0.3)
    model._noise_override = g["in.u"]
    hist, long_hist, fut = inputs_of(g)
    pred, theta, knn, coef = model(history_data=hist, long_history_data=long_hist, future_data=None, batch_seen=0, epoch=epoch)
    loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(fut[..., [0]], mean, std), theta, knn, coef)
    loss.backward()
    torch.cuda.synchronize()
    saved = model._last["saved_gwnet"].cpu()
    touts = [12, 10, 9, 7, 6, 4, 3]
    masks, rates = [], []
    for i, To in enumerate(touts):
        off = L.lib().step_gwnet_saved_offset(B, N, 1, 0, i)
        m = saved[off:off + B * N * To * 32].view(B, N, To, 32)
        vals = torch.unique(m)
        assert set(round(float(v), 5) for v in vals) <= {0.0, round(1 / 0.7, 5)}, vals
        rates.append(float((m > 0).float().mean()))
        masks.append(m.permute(0, 3, 1, 2).contiguous())          # [b][n][t][c] -> the oracle's [B, C, N, T]
    n_el = sum(mk.numel() for mk in masks)
    rate = sum(r * mk.numel() for r, mk in zip(rates, masks)) / n_el
    assert abs(rate - 0.7) < 5 * (0.21 / n_el) ** 0.5 + 1e-3, (rate, rates)
    masks.append(None)
    P = Lh // 12
    hid = model._last["hidden_bf16"].float().cpu().view(B, N, P, 96)
    p = params_of(g)
    o_pred, o_theta, o_knn, o_coef = O.step_forward(g["in.hist"], g["in.long_hist0"].unsqueeze(-1), g["in.node_feats"], p, g["in.u"],
                                                    k, epoch, training=True, hidden=hid, drop_masks=masks,
                                                    hidden_last=model._last["hidden_last"].cpu().view(B, N, 96))
    o_loss = O.step_loss(O.rescale(o_pred, mean, std), O.rescale(g["in.future"][..., [0]], mean, std), o_theta, o_knn, o_coef)
    o_loss.backward()
    nodrop, _, _, _ = O.step_forward(g["in.hist"], g["in.long_hist0"].unsqueeze(-1), g["in.node_feats"], params_of(g), g["in.u"],
                                     k, epoch, training=True, hidden=hid, hidden_last=model._last["hidden_last"].cpu().view(B, N, 96))
    e_pred, moved = rel_l2(pred.detach().cpu(), o_pred), rel_l2(o_pred, nodrop)
    worst, wname = 0.0, ""
    for kname, t in dict(model._trainable()).items():
        og = p[ref_name(kname)].grad
        if float(og.abs().max()) < 1e-4:
            assert max_abs(t.grad.cpu(), og) < 2e-4, kname
            continue
        e = rel_l2(t.grad.cpu(), og)
        if e > worst:
            worst, wname = e, kname
    print(f"{name} gcn dropout on (keep rate {rate:.4f}): pred rel-L2 vs oracle with the same masks {e_pred:.2e} (dropout moves the prediction by "
          f"{moved:.3f}), loss {float(loss):.5f} vs {float(o_loss):.5f}, worst gradient {wname} {worst:.2e}")
    assert e_pred < 2e-3 and moved > 20 * e_pred
    assert float(loss) == pytest.approx(float(o_loss), rel=2e-3)
    assert worst < 1e-2


def test_prefetched_frozen_branch_is_bit_identical():
    """STEP.prefetch(): the frozen branch (TSFormer encoder with dropout on + kNN prior) of the NEXT batch queued on its own stream
    before the current batch's backward.  (a) The branch itself: same launch counter -> the prefetched hidden states and last-patch
    states are BIT-identical to the inline ones, the kNN graph identical (its cosine Gram may use split-K atomics: compared to
    1e-6 / threshold ties).  (b) Three training steps on three different batches, inline vs one step ahead, identically seeded:
    every prediction, graph, loss and parameter agrees to accumulation-order round-off (the backward uses atomics, so two INLINE
    runs differ by as much).  (c) A prefetch for a batch that is then NOT the one passed to forward() is ignored."""
    g = load_golden("step_tiny")
    N, L, T, B, k, epoch, tr = [int(x) for x in g["meta"]]
    mean, std = [float(x) for x in g["meta.scaler"]]
    hist, long_hist, fut = inputs_of(g)
    gen = torch.Generator().manual_seed(3)
    batches = [(hist, long_hist, fut)]
    for _ in range(3):
        lh = long_hist.clone()
        lh[..., 0] = lh[..., 0] + 0.3 * torch.randn(lh[..., 0].shape, generator=gen).cuda()
        batches.append((hist + 0.1 * torch.randn(hist.shape, generator=gen).cuda(), lh, fut))
    # ---- (a)
    torch.manual_seed(99)
    model = build_native(g)
    model.train()
    model.tsformer._seed_counter = 41
    inline = model._frozen_branch(batches[1][1], B, N)
    torch.cuda.synchronize()
    model.tsformer._seed_counter = 41
    model.prefetch(batches[1][1])
    rec = model._take_prefetched(batches[1][1])
    assert rec is not None and model._prefetched is None
    torch.cuda.current_stream().wait_event(rec["done"])
    torch.cuda.synchronize()
    assert torch.equal(rec["enc"]["hidden_bf16"], inline["enc"]["hidden_bf16"]) and torch.equal(rec["enc"]["last"], inline["enc"]["last"])
    assert rel_l2(rec["sim"].cpu(), inline["sim"].cpu()) < 1e-6 and int((rec["adj_knn"] != inline["adj_knn"]).sum()) <= 2
    model.prefetch(batches[2][1])
    # another batch: not used -- and not dropped either: the queue is a short FIFO (the branch of batch i + 1 may be announced before
    # forward() has consumed the one of batch i), a record nobody comes for is evicted by the second prefetch after it or by cancel_prefetch()
    assert model._take_prefetched(batches[1][1]) is None and len(model._prefetched) == 1
    model.prefetch(batches[3][1])
    rec3 = None
    assert model._take_prefetched(batches[3][1]) is not None and model._prefetched is None   # found behind the stale record, which is dropped
    model.prefetch(batches[2][1])
    model.cancel_prefetch()
    assert model._prefetched is None
    torch.cuda.synchronize()

    # ---- (b), (c)
    def run(prefetch, wrong_announcement=False, dropout=True):
        torch.manual_seed(1234)
        model = build_native(g)
        model.train()                                  # dropout on in both the encoder and the gcn layers: seeds matter
        if not dropout:
            model.backend.dropout, model.tsformer.dropout_p = 0.0, 0.0
        model.gumbel_noise = "device"
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=2e-3)
        outs = []
        for i in range(3):
            h, lh, f = batches[i]
            opt.zero_grad(set_to_none=True)
            pred, theta, knn, coef = model(history_data=h, long_history_data=lh, future_data=None, batch_seen=i, epoch=1)
            if prefetch:
                model.prefetch(batches[i + 1][1] if not wrong_announcement else batches[(i + 2) % 4][1])
            loss = O.step_loss(O.rescale(pred[..., [0]], mean, std), O.rescale(f[..., [0]], mean, std), theta, knn, coef)
            loss.backward()
            opt.step()
            outs.append((pred.detach().clone(), theta.detach().clone(), knn.clone(), loss.detach().clone()))
        torch.cuda.synchronize()
        return outs, [p.detach().clone() for p in params], model

    def close(x, y, px, py, what, params=True):
        worst = 0.0
        for (p0, t0, k0, l0), (p1, t1, k1, l1) in zip(x, y):
            worst = max(worst, rel_l2(p1.cpu(), p0.cpu()), rel_l2(t1.cpu(), t0.cpu()), abs(float(l1 - l0)) / abs(float(l0)))
            assert int((k0 != k1).sum()) <= 4
        wp = max(rel_l2(b_.cpu(), a_.cpu()) for a_, b_ in zip(px, py))
        print(f"{what}: worst prediction / theta / loss difference over 3 steps {worst:.2e}, worst parameter {wp:.2e}")
        return max(worst, wp) if params else worst
    a, pa, _ = run(False)
    a2, pa2, _ = run(False)
    b, pb, mb = run(True)
    assert mb._prefetched is not None                  # the last announcement is still pending
    noise = close(a, a2, pa, pa2, "inline vs inline (atomics)")
    assert close(a, b, pa, pb, "inline vs prefetched") <= max(10 * noise, 1e-5)
    # announced batches that never match: forward() must ignore them and take the inline path.  The extra encoder launches consume
    # dropout seeds, so the comparison is made with dropout off
    d0, pd0, _ = run(False, dropout=False)
    d1, pd1, _ = run(True, wrong_announcement=True, dropout=False)
    # (parameters are not compared here: with dropout off the biases in front of a BatchNorm have an exactly cancelling gradient,
    # i.e. pure round-off whose SIGN Adam turns into a full +-lr update -- two inline runs differ there just as much)
    assert close(d0, d1, pd0, pd1, "inline vs mismatching announcements (dropout off)", params=False) <= max(10 * noise, 1e-5)


def test_standalone_submodule_forwards_match_oracle():
    """The reference's sub-modules are callable on their own (graphwavenet/model.py:132, discrete_graph_learning.py:113); the native
    ones are too, forward-only: GraphWaveNet(input, hidden_states, sampled_adj) -> [B, N, 12] and DiscreteGraphLearning(long_history,
    tsformer) -> (logits, hidden, adj_knn, sampled_adj), both against the oracle in eval mode (running statistics, no dropout) with
    the same host-drawn Gumbel noise; gradients are refused outside torch.no_grad()."""
    g = load_golden("step_tiny")
    N, L, T, B, k, epoch, tr = [int(x) for x in g["meta"]]
    model = build_native(g)
    model.eval()
    p = params_of(g, requires_grad=False)
    hist, long_hist, fut = inputs_of(g)
    with pytest.raises(RuntimeError, match="forward-only"):
        model.backend(hist, torch.zeros(B, N, 96, device="cuda"), torch.zeros(B, N, N, device="cuda"))
    with torch.no_grad():
        torch.manual_seed(77)
        logits, hidden, knn, samp = model.discrete_graph_learning(long_hist, model.tsformer)
        pred = model.backend(hist, hidden[:, :, -1, :].contiguous(), samp)
    torch.manual_seed(77)
    u = torch.rand(B, N * N, 2)
    hid = hidden.cpu()
    o_logits, _, o_knn, o_samp = O.dgl_forward(g["in.long_hist0"], g["in.node_feats"], p, u, k, training=False, hidden=hid)
    theta, o_theta = torch.softmax(logits.cpu(), -1)[..., 0], torch.softmax(o_logits, -1)[..., 0]
    assert logits.shape == (B, N * N, 2) and hidden.shape == (B, N, L // 12, 96) and pred.shape == (B, N, 12)
    assert max_abs(theta, o_theta) < 2e-5
    assert torch.equal(samp.cpu(), o_samp)
    assert int((knn.cpu() != o_knn).sum()) <= 4                                # threshold ties of the bf16 Gram
    o_pred = O.gwnet_forward(g["in.hist"], hid[:, :, -1, :], o_samp, p, training=False)
    e = rel_l2(pred.cpu(), o_pred)
    print(f"standalone sub-modules (eval): theta max-abs {max_abs(theta, o_theta):.1e}, prediction rel-L2 vs oracle {e:.2e}")
    assert e < 1e-4
