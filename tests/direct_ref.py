"""Direct drivers and float64 references of the GraphWaveNet backbone and of the graph learner's edge kernels.

Shared by tests/test_gpu_gwnet_direct.py, tests/test_gpu_dgl_edges_direct.py (device side: ``run_gwnet`` / ``run_edges`` call
``step_gwnet_{forward,backward}`` / ``step_dgl_edges_{forward,backward}`` through ctypes, outside ``step_amd.STEP``) and
tests/test_direct_ref_host.py (which pins ``gwnet_ref`` / ``edges_ref`` to the reference's golden numbers).  The references are
``oracle/step_oracle.py`` under autograd in the requested dtype; nothing here restates arithmetic a second time, except the bf16
operand models: that of the diffusion hop (``_RoundedHop``), which follows ``nconv_fwd3`` / ``nconv_bwd_data3`` / the adjacency-gradient
contraction of ``step_amd/csrc/gwnet.hip``: those three products round BOTH operands to bf16 (round to nearest even: the support
stack through ``stacks_to_bf16_kernel``, the slot operand in ``step_gemm``'s bf16 path or ``slots_to_bf16T_kernel``) and accumulate in
f32; what they write (the hop outputs in the gcn buffer, the gradient slots, the support gradients) stays f32 and is rounded again
only where the next such product reads it.  ``_RoundedContractions`` extends the same treatment to the other contractions that
``StepGwnetParams.gemm_bf16 = 1`` moves to the bf16 matrix cores (gated TCN, skip / mix / end convolutions, fc_his): the flag switches
them all, so a model of the hops alone is not a model of what the device computes in that mode.

FLOOR_REL / FLOOR_ABS: the run-to-run noise of the kernels' float32 atomics, measured by test_buffers_can_be_reused (largest
difference between two runs in fresh buffers: 1.78e-6 relative L2 on start_b, 1.71e-6 max-abs on an analytically zero gcn bias).
"""
import contextlib
import ctypes
import functools

import torch

from oracle import step_oracle as O

FLOOR_REL, FLOOR_ABS = 1.8e-6, 1.8e-6
TOUT = (12, 10, 9, 7, 6, 4, 3, 1)          # time steps of the eight layers' outputs (13 -> dilations 1, 2, 1, 2, ...)
EDGE_PRE = "discrete_graph_learning."
TEMPERATURE = 0.5
MOMENTUM = 0.1


# ----------------------------------------------------------------------------------------- metrics
def rel_l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def max_abs(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


class Compare:
    """The tolerance rule of the direct tests: for every tensor e_dev = err(device, f64) <= M * err(f32 oracle, f64) + floor, with
    err = relative L2, or the max-abs difference for a tensor that is zero in exact arithmetic (|f64| <= 1e-6 everywhere: the gcn
    biases in front of a train-mode BatchNorm).  Every figure is printed before anything is asserted; ``finish`` asserts."""
    ZERO = 1e-6

    def __init__(self, tag, M, floor, floor_abs):
        self.tag, self.M, self.floor, self.floor_abs = tag, M, floor, floor_abs
        self.bad, self.worst = [], 0.0

    def add(self, name, dev, r64, r32, extra=0.0, extra_abs=0.0, report_only=False):
        assert tuple(dev.shape) == tuple(r64.shape), (name, tuple(dev.shape), tuple(r64.shape))
        assert bool(torch.isfinite(dev).all()), f"{self.tag} {name}: device result is not finite"
        zero = float(r64.abs().max()) <= self.ZERO
        err = max_abs if zero else rel_l2
        e_dev, e_f32 = err(dev, r64), err(r32, r64)
        bound = self.M * e_f32 + (self.floor_abs + extra_abs if zero else self.floor + extra)
        ratio = e_dev / e_f32 if e_f32 > 0 else float("inf") if e_dev > 0 else 0.0
        self.worst = max(self.worst, ratio if e_dev > (self.floor_abs if zero else self.floor) else 0.0)
        print(f"RATIO {self.tag} {name:<14s} {'maxabs' if zero else 'rel_l2'} e_dev={e_dev:.3e} e_f32={e_f32:.3e} ratio={ratio:8.2f} bound={bound:.3e}"
              + ("" if e_dev <= bound else "   <-- ABOVE"))
        if not e_dev <= bound and not report_only:
            self.bad.append((name, e_dev, e_f32, bound))

    def finish(self):
        print(f"RATIO {self.tag} worst ratio above the floor: {self.worst:.2f}")
        assert not self.bad, (self.tag, self.bad)


# ----------------------------------------------------------------------------------------- parameters and inputs
def native_key(name):
    """name of GraphWaveNet.native_tensors() -> state_dict key"""
    base, _, idx = name.partition(".")
    kind = {"_w": "weight", "_b": "bias", "_rm": "running_mean", "_rv": "running_var"}
    for suf, attr in kind.items():
        if base.endswith(suf):
            stem = base[:-len(suf)]
            break
    else:
        return base          # nodevec1 / nodevec2
    mod = {"start": "start_conv", "filter": f"filter_convs.{idx}", "gate": f"gate_convs.{idx}", "skip": f"skip_convs.{idx}",
           "bn": f"bn.{idx}", "gconv": f"gconv.{idx}.mlp.mlp", "fc_his0": "fc_his.0", "fc_his2": "fc_his.2", "end1": "end_conv_1",
           "end2": "end_conv_2"}[stem]
    return f"{mod}.{attr}"


def gwnet_state(N, seed):
    """state_dict of a freshly initialised GraphWaveNet (the module's own init) with every BatchNorm tensor moved off 1 / 0 / 0 / 1."""
    from step_amd.step_arch.graphwavenet import GraphWaveNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        sd = {k: v.detach().clone() for k, v in GraphWaveNet(num_nodes=N, support_len=2).state_dict().items()}
    g = torch.Generator().manual_seed(seed + 77)
    for i in range(8):
        sd[f"bn.{i}.weight"] = 0.5 + torch.rand(32, generator=g)
        sd[f"bn.{i}.bias"] = 0.3 * torch.randn(32, generator=g)
        sd[f"bn.{i}.running_mean"] = 0.2 * torch.randn(32, generator=g)
        sd[f"bn.{i}.running_var"] = 0.5 + torch.rand(32, generator=g)
    return sd


def gwnet_case(B, N, seed=0, weighted=False, cin=2):
    """inputs of one backbone call: hist [B,12,N,cin], last [B,N,96], adj [B,N,N], dpred [B,12,N] and the parameters"""
    g = torch.Generator().manual_seed(1000 * seed + 17 * N + B)
    hist = torch.randn(B, 12, N, cin, generator=g)
    last = torch.randn(B, N, 96, generator=g)
    if weighted:          # non-negative real weights, the diagonal included
        adj = torch.rand(B, N, N, generator=g) * (torch.rand(B, N, N, generator=g) < 0.4).float()
        adj = adj + torch.diag_embed(0.25 + torch.rand(B, N, generator=g))
    else:
        adj = (torch.rand(B, N, N, generator=g) < 0.4).float() * (1 - torch.eye(N))
    dpred = torch.randn(B, 12, N, generator=g)
    return {"B": B, "N": N, "hist": hist, "last": last, "adj": adj, "dpred": dpred, "sd": gwnet_state(N, seed + N)}


def edge_case(B, N, seed=0):
    """edge-half parameters from a seeded generator, a unit-variance global feature (it is a BatchNorm output), noise and gradients"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * N + B)
    ep = {"fc_out_w": torch.randn(100, 200, generator=g) * 0.07, "fc_out_b": torch.randn(100, generator=g) * 0.1,
          "fc_cat_w": torch.randn(2, 100, generator=g) * 0.1, "fc_cat_b": torch.randn(2, generator=g) * 0.1}
    gf = torch.randn(N, 100, generator=g)
    u = torch.rand(B, N * N, 2, generator=g)
    # the ends of torch.rand's range at known places: 0 and the largest float32 below 1
    flat = u.view(-1)
    top = 1.0 - 2.0 ** -24
    for pos, val in ((0, 0.0), (1, top), (2, top), (3, 0.0), (flat.numel() - 1, 0.0), (flat.numel() - 2, top), (flat.numel() // 2, 0.0)):
        flat[pos] = val
    dtheta = torch.randn(B, N, N, generator=g)
    dadj = torch.randn(B, N, N, generator=g)
    dadj = dadj + torch.diag_embed(torch.full((B, N), 1e30))          # the diagonal of the sample is cleared: this must have no effect
    return {"B": B, "N": N, "ep": ep, "g": gf, "u": u, "dtheta": dtheta, "dadj": dadj}


# ----------------------------------------------------------------------------------------- bf16 operand model of the hop
def round_bf16(t):
    """what a device f32 value becomes as a bf16 matrix-core operand (round to nearest even), kept in t's dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _RoundedHop(torch.autograd.Function):
    """out[n,c,w,l] = sum_v x[n,c,v,l] a[n,v,w] with the operand rounding of gwnet.hip's three hop products; products and sums in the
    tensors' own dtype (float64 in the tests).  forward = nconv_fwd3 (support and slot rounded); d x = nconv_bwd_data3 (support and
    gradient slot rounded); d a = the adjacency-gradient contraction (saved slot and gradient slot rounded)."""

    @staticmethod
    def forward(ctx, x, a, rnd):
        ctx.save_for_backward(x, a)
        ctx.rnd = rnd
        return torch.einsum("ncvl,nvw->ncwl", rnd(x), rnd(a))

    @staticmethod
    def backward(ctx, dout):
        x, a = ctx.saved_tensors
        rnd = ctx.rnd
        dx = torch.einsum("ncwl,nvw->ncvl", rnd(dout), rnd(a))
        da = torch.einsum("ncvl,ncwl->nvw", rnd(x), rnd(dout))
        return dx, da, None


class _RoundedConv(torch.autograd.Function):
    """out = einsum("oc,bcnt->bont", w, x) (a 1x1 convolution / one tap of the gated TCN) as a bf16-mode contraction: the forward product,
    the data gradient and the weight gradient each round both of their operands (tcn_fwd / tcn_bwd / mix_fwd / mix_bwd with BF16, step_gemm
    with compute_bf16).  round_bwd = False: the two backward products stay f32 (end_conv_2: gwnet.hip leaves d_e1 and dW2 without
    compute_bf16)."""

    @staticmethod
    def forward(ctx, w, x, rnd, round_bwd):
        ctx.save_for_backward(w, x)
        ctx.rnd = rnd if round_bwd else (lambda t: t)
        return torch.einsum("oc,bcnt->bont", rnd(w), rnd(x))

    @staticmethod
    def backward(ctx, dy):
        w, x = ctx.saved_tensors
        rnd = ctx.rnd
        return torch.einsum("bont,bcnt->oc", rnd(dy), rnd(x)), torch.einsum("oc,bont->bcnt", rnd(w), rnd(dy)), None, None


class _RoundedLinear(torch.autograd.Function):
    """x [..., K] @ wt [K, M] as a bf16-mode contraction (the fc_his branch: forward, data and weight gradient all with compute_bf16)"""

    @staticmethod
    def forward(ctx, x, wt, rnd):
        ctx.save_for_backward(x, wt)
        ctx.rnd = rnd
        return torch.matmul(rnd(x), rnd(wt))

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        rnd = ctx.rnd
        K, Mo = wt.shape
        return torch.matmul(rnd(dy), rnd(wt).transpose(0, 1)), torch.matmul(rnd(x).reshape(-1, K).transpose(0, 1), rnd(dy).reshape(-1, Mo)), None


class _RoundedGrad(torch.autograd.Function):
    """identity whose gradient is rounded: a bias gradient that step_gemm forms as the row sums of its (rounded) A operand"""

    @staticmethod
    def forward(ctx, x, rnd):
        ctx.rnd = rnd
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        return ctx.rnd(dy), None


class _RoundedContractions(torch.overrides.TorchFunctionMode):
    """While O.gwnet_forward runs: every contraction that bf16 mode (StepGwnetParams.gemm_bf16 = 1) puts on the bf16 matrix cores takes
    rounded operands -- the gated TCN taps, the skip and mix convolutions, end_conv_1, end_conv_2 (forward only) and the two fc_his
    layers.  What gwnet.hip keeps in f32 stays as the oracle has it: the start convolution (K = 2, a plain kernel), the node-embedding
    product (K = 10) and both backward products of end_conv_2.  The bias gradients of the gated TCN, the gcn mix and end_conv_1 are the
    row sums of the weight-gradient product's rounded operand (StepGemm.a_rowsum: a column of ones through the matrix core), so they
    sum rounded values: that is all there is to the gcn biases' gradients, which are zero in exact arithmetic."""
    _ADD = (torch.add, torch.Tensor.add, torch.Tensor.__add__)

    def __init__(self, rnd):
        super().__init__()
        self.rnd, self.count = rnd, 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.einsum and args[0] == "oc,bcnt->bont" and args[1].shape[1] != 2:          # (in = 2: the start convolution)
            self.count += 1
            return _RoundedConv.apply(args[1], args[2], self.rnd, tuple(args[1].shape) != (12, 512))
        if func in (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__) and args[0].shape[-1] != 10:          # (K = 10: the node embeddings)
            self.count += 1
            return _RoundedLinear.apply(args[0], args[1], self.rnd)
        if func in self._ADD and len(args) == 2 and all(isinstance(a, torch.Tensor) and a.dim() == 4 for a in args):
            y, b = args
            # a [1, C, 1, 1] bias on a convolution's output; C = 32: gated TCN / gcn mix, 512: end_conv_1 (T = 13 is the start convolution's
            # output, whose gradients a plain f32 kernel sums; the skip biases -- 256 -- and end_conv_2's -- 12 -- are f32 column sums)
            if b.requires_grad and b.shape[0] == 1 and tuple(b.shape[2:]) == (1, 1) and b.shape[1] in (32, 512) and y.shape[3] != 13:
                return func(y, _RoundedGrad.apply(b.expand_as(y), self.rnd), **kwargs)
        return func(*args, **kwargs)


@contextlib.contextmanager
def hop_model(kind):
    """kind: None (the oracle as it is); "bf16": the three hop products round their operands; "bf16_all": so does every other
    contraction of bf16 mode (_RoundedContractions); "exact" / "exact_all": the same autograd.Functions with rounding switched off"""
    if kind is None:
        yield
        return
    rnd = round_bf16 if kind.startswith("bf16") else (lambda t: t)

    def nconv(x, a):
        if a.dim() == 2:          # the adaptive support: replicated per sample on the device, its gradient summed over the samples
            a = a.unsqueeze(0).expand(x.shape[0], -1, -1)
        return _RoundedHop.apply(x, a, rnd)
    plain, O.nconv = O.nconv, nconv
    try:
        if kind.endswith("_all"):
            with _RoundedContractions(rnd) as mode:
                yield
            assert mode.count == 7 * 6 + 5 + 2 + 2, mode.count          # 4 taps + skip (+ mix) per layer, end_conv_1 / _2, fc_his.0 / .2
        else:
            yield
    finally:
        O.nconv = plain


# ----------------------------------------------------------------------------------------- references
def gwnet_ref(dtype, sd, hist, last, adj, dpred, training=True, drop_masks=None, hop=None, names=None):
    """O.gwnet_forward under autograd in ``dtype`` with loss sum(pred * dpred).  sd: state_dict keys (no prefix).  drop_masks: list of
    the seven layers' masks [B,32,N,T_i], already scaled by 1 / keep.  -> {"pred" [B,12,N], "dadj", "grads": native name -> gradient,
    "running": native name -> updated running statistic (momentum 0.1, unbiased variance)}"""
    p = {}
    for k, v in sd.items():
        if v.is_floating_point():
            p["backend." + k] = v.detach().to(dtype).clone().requires_grad_("running_" not in k)
    a = adj.detach().to(dtype).clone().requires_grad_(True)
    masks = None if drop_masks is None else [m.to(dtype) for m in drop_masks]
    stats = {}
    with hop_model(hop):
        pred = O.gwnet_forward(hist[..., :2].to(dtype), last.to(dtype), a, p, training=training, drop_masks=masks, stats=stats).transpose(1, 2)
    (pred * dpred.to(dtype)).sum().backward()
    grads, running = {}, {}
    if names is None:
        names = [n for n in _all_native_names() if "_rm" not in n and "_rv" not in n and not (n.endswith(".7") and n.split(".")[0] in
                                                                                               ("gconv_w", "gconv_b", "bn_w", "bn_b"))]
    for n in names:
        gr = p["backend." + native_key(n)].grad
        assert gr is not None, n
        grads[n] = gr
    for i in range(8):
        rm, rv = p[f"backend.bn.{i}.running_mean"], p[f"backend.bn.{i}.running_var"]
        if training and f"bn.{i}" in stats:
            mu, var_u = stats[f"bn.{i}"]
            rm, rv = (1 - MOMENTUM) * rm + MOMENTUM * mu, (1 - MOMENTUM) * rv + MOMENTUM * var_u
        running[f"bn_rm.{i}"], running[f"bn_rv.{i}"] = rm.detach(), rv.detach()
    return {"pred": pred.detach(), "dadj": a.grad, "grads": grads, "running": running}


def _all_native_names():
    names = ["nodevec1", "nodevec2", "start_w", "start_b", "fc_his0_w", "fc_his0_b", "fc_his2_w", "fc_his2_b", "end1_w", "end1_b",
             "end2_w", "end2_b"]
    for i in range(8):
        names += [f"{k}.{i}" for k in ("filter_w", "filter_b", "gate_w", "gate_b", "skip_w", "skip_b", "bn_w", "bn_b", "bn_rm", "bn_rv",
                                       "gconv_w", "gconv_b")]
    return names


EDGE_VARIANTS = ("both", "dtheta", "dadj")          # which of dtheta / dadj the backward is given (the other one is NULL)


def edges_ref(dtype, ep, g, u, dtheta=None, dadj=None, temperature=TEMPERATURE, variant=None):
    """O.dgl_edge_logits + the Gumbel soft sample in ``dtype``.  The noise gets its eps in float32, as the reference program adds it
    (torch.rand is float32), and is cast afterwards; everything after that is in ``dtype``.  -> {"theta" [B,N,N],
    "a0" [B,N,N] = (l0 + g0) - (l1 + g1)} and, with a variant, the gradients "dg", "fc_out_w", "fc_out_b", "fc_cat_w", "fc_cat_b" of
    sum(theta * dtheta) ("dtheta"), sum(samp * dadj) ("dadj") or their sum ("both"), samp = soft sample * (1 - eye)."""
    B, N = u.shape[0], g.shape[0]
    need = variant is not None
    p = {EDGE_PRE + {"fc_out_w": "fc_out.weight", "fc_out_b": "fc_out.bias", "fc_cat_w": "fc_cat.weight", "fc_cat_b": "fc_cat.bias"}[k]:
         v.detach().to(dtype).clone().requires_grad_(need) for k, v in ep.items()}
    gf = g.detach().to(dtype).clone().requires_grad_(need)
    ue = u.to(torch.float32) + 1e-10          # float32, like the reference
    with torch.set_grad_enabled(need):
        logits = O.dgl_edge_logits(gf, p, EDGE_PRE, row_chunk=128 if N > 300 else None).unsqueeze(0).expand(B, N * N, 2)
        gmb = -torch.log(-torch.log(ue.to(dtype)) + 1e-10)
        a0 = ((logits[..., 0] + gmb[..., 0]) - (logits[..., 1] + gmb[..., 1])).detach().reshape(B, N, N)
        theta = torch.softmax(logits, -1)[..., 0].reshape(B, N, N)
        out = {"theta": theta.detach(), "a0": a0}
        if not need:
            return out
        loss = 0
        if variant in ("both", "dtheta"):
            loss = loss + (theta * dtheta.to(dtype)).sum()
        if variant in ("both", "dadj"):
            y = torch.softmax((logits + gmb) / temperature, -1)
            samp = y[..., 0].reshape(B, N, N) * (1 - torch.eye(N, dtype=dtype))
            loss = loss + (samp * dadj.to(dtype)).sum()
    wrt = [gf] + [p[EDGE_PRE + k] for k in ("fc_out.weight", "fc_out.bias", "fc_cat.weight", "fc_cat.bias")]
    out.update(zip(("dg", "fc_out_w", "fc_out_b", "fc_cat_w", "fc_cat_b"), torch.autograd.grad(loss, wrt)))
    return out


# ----------------------------------------------------------------------------------------- device drivers
def _nan_floats(n, dev):
    """n floats of 0xFF bytes (NaN): the product hands the library torch.empty memory, so arbitrary contents are the contract"""
    return torch.empty(int(n) * 4, dtype=torch.uint8, device=dev).fill_(0xFF).view(torch.float32)


def _vp(stream):
    return None if stream is None else ctypes.c_void_p(stream.cuda_stream)


def run_gwnet(case, training=1, bf16=0, dropout_p=0.0, seed=20240607, grad_fill=None, streams=None, buffers=None, hist=None, repeat=1,
              backward=True):
    """step_gwnet_forward + step_gwnet_backward on the case's inputs, every scratch and output buffer pre-filled with NaN bytes.
    grad_fill: native name -> G0 the gradient buffers start from (None: zeros; the backward accumulates).  streams: None (aux / leaf NULL)
    or (aux, leaf) torch streams, joined before anything is read.  buffers: (saved, work_fwd, work_bwd) of an earlier call to run in
    again.  repeat: forward + backward this many times in the same buffers (gradients and statistics reset in between); the last one
    is returned.  -> host copies: pred [B,12,N], dadj, grads, running (bn_rm / bn_rv .0-.7), masks (list of [B,32,N,T_i]) with dropout."""
    from step_amd import _lib as L
    from step_amd.step_arch.graphwavenet import GraphWaveNet, fill_gwnet_struct
    dev = torch.device("cuda")
    B, N = case["B"], case["N"]
    hist = (case["hist"] if hist is None else hist).to(dev).contiguous()
    cin = hist.shape[3]
    last, adj, dpred = (case[k].to(dev).contiguous() for k in ("last", "adj", "dpred"))
    with torch.random.fork_rng(devices=[]):
        m = GraphWaveNet(num_nodes=N, support_len=2)
    m.load_state_dict(case["sd"])
    m = m.to(dev)
    nt = m.native_tensors()
    struct = fill_gwnet_struct(nt, bf16)
    drop = int(bool(training) and dropout_p > 0)
    lib = L.lib()
    if buffers is None:
        buffers = (_nan_floats(lib.step_gwnet_saved_floats(B, N, drop), dev), _nan_floats(lib.step_gwnet_work_floats(B, N, 0), dev),
                   _nan_floats(lib.step_gwnet_work_floats(B, N, 1), dev))
    saved, wfwd, wbwd = buffers
    names = list(m.trainable_native())
    initial = {k: nt[k].detach().clone() for k in nt if "_rm" in k or "_rv" in k}
    for _ in range(repeat):
        for k, v in initial.items():
            nt[k].copy_(v)
        pred = _nan_floats(B * 12 * N, dev).view(B, 12, N)
        dadj = _nan_floats(B * N * N, dev).view(B, N, N)
        grads = {k: (torch.zeros_like(nt[k]) if grad_fill is None else grad_fill[k].to(dev).contiguous().clone()) for k in names}
        gstruct = fill_gwnet_struct(grads, bf16)
        st = L.stream()
        L.call("step_gwnet_forward", L.ptr(hist), B, N, cin, L.ptr(last.view(B * N, 96)), L.ptr(adj), ctypes.byref(struct), int(training),
               float(dropout_p), seed, MOMENTUM, L.ptr(saved), L.ptr(wfwd), L.ptr(pred), st)
        aux, leaf = streams if streams is not None else (None, None)
        if not backward:          # (an evaluation forward keeps no batch statistics for a backward)
            torch.cuda.synchronize()
            return {"pred": pred.cpu(), "running": {k: nt[k].detach().cpu() for k in initial}, "initial": {k: v.cpu() for k, v in initial.items()}}
        L.call("step_gwnet_backward", L.ptr(hist), B, N, cin, L.ptr(last.view(B * N, 96)), ctypes.byref(struct), L.ptr(saved), L.ptr(wbwd),
               L.ptr(dpred), ctypes.byref(gstruct), L.ptr(dadj), drop, _vp(aux), _vp(leaf), st)
        for s in (aux, leaf):          # the leaves are not joined inside the call: the first reader of the gradients waits for them
            if s is not None:
                torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
    out = {"pred": pred.cpu(), "dadj": dadj.cpu(), "grads": {k: v.cpu() for k, v in grads.items()},
           "running": {k: nt[k].detach().cpu() for k in initial}, "initial": {k: v.cpu() for k, v in initial.items()}, "buffers": buffers}
    if drop:
        out["masks"] = []
        for i in range(7):
            off = lib.step_gwnet_saved_offset(B, N, 1, 0, i)
            assert off >= 0
            out["masks"].append(saved[off:off + B * N * TOUT[i] * 32].view(B, N, TOUT[i], 32).permute(0, 3, 1, 2).contiguous().cpu())
    return out


def run_edges(case, use_u=True, seed=1, variant="both", grad_fill=None, aux=None, backward=True):
    """step_dgl_edges_forward (+ step_dgl_edges_backward) with theta_out = saved + step_dgl_edges_theta_offset(N), as step.py passes it,
    every scratch and output buffer pre-filled with NaN bytes (dg too: the backward STORES it -- its first product into dg does not
    accumulate, and step.py hands it torch.empty memory).  grad_fill: name -> G0 of the four weight gradients (they accumulate).
    -> host copies of theta, adj, y0 (the soft sample), dg and the four gradients."""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    dev = torch.device("cuda")
    B, N = case["B"], case["N"]
    lib = L.lib()
    ep = {k: v.to(dev).contiguous() for k, v in case["ep"].items()}
    struct = fill_dgl_struct(ep, 0)
    g = case["g"].to(dev).contiguous()
    u = case["u"].to(dev).contiguous() if use_u else None
    saved = _nan_floats(lib.step_dgl_edges_saved_floats(B, N), dev)
    to = int(lib.step_dgl_edges_theta_offset(N))
    theta = saved[to:to + B * N * N].view(B, N, N)
    y0 = saved[to + B * N * N:to + 2 * B * N * N].view(B, N, N)
    adj = _nan_floats(B * N * N, dev).view(B, N, N)
    st = L.stream()
    L.call("step_dgl_edges_forward", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(u), seed, TEMPERATURE, L.ptr(saved), L.ptr(theta), L.ptr(adj), st)
    torch.cuda.synchronize()
    out = {"theta": theta.cpu(), "adj": adj.cpu(), "y0": y0.cpu()}
    if not backward:
        return out
    work = _nan_floats(lib.step_dgl_edges_work_floats(N), dev)
    grads = {k: (torch.zeros_like(v) if grad_fill is None else grad_fill[k].to(dev).contiguous().clone()) for k, v in ep.items()}
    gstruct = fill_dgl_struct(grads, 0)
    dg = _nan_floats(N * 100, dev).view(N, 100)
    dtheta = case["dtheta"].to(dev).contiguous() if variant in ("both", "dtheta") else None
    dadj = case["dadj"].to(dev).contiguous() if variant in ("both", "dadj") else None
    L.call("step_dgl_edges_backward", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(saved), L.ptr(dtheta), L.ptr(dadj), TEMPERATURE,
           L.ptr(work), ctypes.byref(gstruct), L.ptr(dg), _vp(aux), st)
    if aux is not None:
        torch.cuda.current_stream().wait_stream(aux)
    torch.cuda.synchronize()
    out["dg"] = dg.cpu()
    out.update({k: v.cpu() for k, v in grads.items()})
    return out


def flat_gwnet(out):
    """every compared tensor of a gwnet result (device or reference) under one name: the prediction and the adjacency gradient whole
    and per sample (one wrong sample must not hide in the aggregate), the gradients, the running statistics of the seven live
    BatchNorms"""
    d = {"pred": out["pred"], "dadj": out["dadj"]}
    for b in range(out["pred"].shape[0]):
        d[f"pred[{b}]"], d[f"dadj[{b}]"] = out["pred"][b], out["dadj"][b]
    d.update(out["grads"])
    for i in range(7):
        d[f"bn_rm.{i}"], d[f"bn_rv.{i}"] = out["running"][f"bn_rm.{i}"], out["running"][f"bn_rv.{i}"]
    return d


# ----------------------------------------------------------------------------------------- shared, cached references
@functools.lru_cache(maxsize=None)
def cached_gwnet_case(B, N, weighted=False):
    return gwnet_case(B, N, weighted=weighted)


@functools.lru_cache(maxsize=None)
def cached_gwnet_ref(B, N, dtype, hop=None, weighted=False, training=True):
    """the reference of cached_gwnet_case, computed once per process and shared (nobody writes into it)"""
    c = cached_gwnet_case(B, N, weighted)
    return gwnet_ref(dtype, c["sd"], c["hist"], c["last"], c["adj"], c["dpred"], training=training, hop=hop)


@functools.lru_cache(maxsize=None)
def cached_edge_case(B, N):
    return edge_case(B, N)


@functools.lru_cache(maxsize=None)
def cached_edges_ref(B, N, dtype, variant=None):
    c = cached_edge_case(B, N)
    return edges_ref(dtype, c["ep"], c["g"], c["u"], c["dtheta"], c["dadj"], variant=variant)
