"""Direct drivers and float64 references of the GraphWaveNet backbone and of the graph learner's edge and global-feature kernels.

Shared by tests/test_gpu_gwnet_direct.py, tests/test_gpu_dgl_edges_direct.py, tests/test_gpu_dgl_global_direct.py (device side:
``run_gwnet`` / ``run_edges`` / ``run_global`` / ``run_global_sliced`` call ``step_gwnet_{forward,backward}`` /
``step_dgl_edges_{forward,backward}`` / ``step_dgl_global_*`` through ctypes, outside ``step_amd.STEP``) and
tests/test_direct_ref_host.py (which pins ``gwnet_ref`` / ``edges_ref`` / ``global_ref`` to the reference's golden numbers).  The references are
``oracle/step_oracle.py`` under autograd in the requested dtype; nothing here restates arithmetic a second time, except the bf16
operand models: that of the diffusion hop (``_RoundedHop``), which follows ``nconv_fwd3`` / ``nconv_bwd_data3`` / the adjacency-gradient
contraction of ``step_amd/csrc/gwnet.hip``: those three products round BOTH operands to bf16 (round to nearest even: the support
stack through ``stacks_to_bf16_kernel``, the slot operand in ``step_gemm``'s bf16 path or ``slots_to_bf16T_kernel``) and accumulate in
f32; what they write (the hop outputs in the gcn buffer, the gradient slots, the support gradients) stays f32 and is rounded again
only where the next such product reads it.  ``_RoundedContractions`` extends the same treatment to the other contractions that
``StepGwnetParams.gemm_bf16 = 1`` moves to the bf16 matrix cores (gated TCN, skip / mix / end convolutions, fc_his): the flag switches
them all, so a model of the hops alone is not a model of what the device computes in that mode.

The global branch has its own operand model, ``global_bf16_model`` (see there).

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


# ----------------------------------------------------------------------------------------- the graph learner's global branch
GLOBAL_TRAINABLE = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "fc_w", "fc_b", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "bn3_w", "bn3_b")
GLOBAL_RUNNING = ("bn1_rm", "bn1_rv", "bn2_rm", "bn2_rv", "bn3_rm", "bn3_rv")
FRESH_FC_GRAD = 16          # STEP_DGL_FRESH_FC_GRAD of include/step_hip.h
GUARD = 4096                # floats of guard band on either side of a buffer handed to the library
_GUARD_FRONT, _GUARD_BACK = 0x5A17C0DE, 0x3C69A5F1


# The shapes (N, T) of tests/test_gpu_dgl_global_direct.py, each on an edge of the kernels (T2 = T - 18, T1 = T - 9): T2 = 1 (the smallest
# the entry point accepts) and 10 (one kernel width); 127 / 128 (three-pass / fused BatchNorm2 backward in f32 mode); 132 with four row
# tiles and a tail; 256 = WG_SC; row-tile tails of the fc GEMMs; 1024 / 1025 = FW_TT (+ 1); 3584 / 3585 = WG_SC x WG_PASSES (+ 1); the two
# shapes of the time-slice cases.  No N below 13 (N = 5 and 7 give a dead BatchNorm3 feature: variance exactly 0).  tests/test_direct_ref_host.py
# holds every one of them to the conditioning the tolerance rule relies on.
GLOBAL_SHAPES = [(33, 19), (33, 28), (13, 145), (13, 146), (260, 150), (13, 274), (70, 300), (131, 300), (13, 600), (70, 600), (13, 1042),
                 (13, 1043), (13, 3602), (13, 3603)]
GLOBAL_FORWARD_ONLY = [(8200, 40)]          # nblk >= 8192 of dgl_bn_stats; float32 autograd on the CPU is itself 1e-3 off on its gradients
GLOBAL_SLICED = [(13, 600, ((0, 291), (291, 582))), (13, 600, ((0, 194), (194, 388), (388, 582))), (13, 600, ((0, 200), (200, 582))),
                 (70, 600, ((0, 291), (291, 582)))]
# the tolerance rule's two numbers for the global branch (measured: docstring of tests/test_gpu_dgl_global_direct.py)
GLOBAL_M, GLOBAL_FLOOR = 8.0, 3.0e-6


def global_key(name):
    """StepDglParams name -> state_dict key (with the prefix the oracle takes)"""
    base, kind = name.rsplit("_", 1)
    return EDGE_PRE + base + {"w": ".weight", "b": ".bias", "rm": ".running_mean", "rv": ".running_var"}[kind]


def global_case(N, T, seed=0):
    """Seeded host tensors of one call of the global branch: the series [N, T] (a daily sine with a per-node phase plus 0.3 noise, the
    recipe of tests/test_gpu_dgl_conv.py, drawn in the same order from the same seed N * 1000 + T), the twelve trainable tensors
    (weights scaled 0.3 / 0.1 / K ** -0.5, BatchNorm weights 0.5 + rand), dg [N, 100], and the six running statistics moved off 0 / 1:
    started at their defaults, a swapped mean / variance or a wrong momentum would go unnoticed."""
    gen = torch.Generator().manual_seed(N * 1000 + T + 104729 * seed)
    tt = torch.arange(T, dtype=torch.float32)
    series = torch.sin(2 * 3.14159265 * tt[None, :] / 288.0 + 6.28 * torch.rand(N, 1, generator=gen)) + 0.3 * torch.randn(N, T, generator=gen)
    K = 16 * (T - 18)
    p = {"conv1_w": torch.randn(8, 1, 10, generator=gen) * 0.3, "conv1_b": torch.randn(8, generator=gen) * 0.1,
         "conv2_w": torch.randn(16, 8, 10, generator=gen) * 0.1, "conv2_b": torch.randn(16, generator=gen) * 0.1,
         "fc_w": torch.randn(100, K, generator=gen) * (1.0 / K ** 0.5), "fc_b": torch.randn(100, generator=gen) * 0.1,
         "bn1_w": torch.rand(8, generator=gen) + 0.5, "bn1_b": torch.randn(8, generator=gen) * 0.1,
         "bn2_w": torch.rand(16, generator=gen) + 0.5, "bn2_b": torch.randn(16, generator=gen) * 0.1,
         "bn3_w": torch.rand(100, generator=gen) + 0.5, "bn3_b": torch.randn(100, generator=gen) * 0.1}
    dg = torch.randn(N, 100, generator=gen)
    for name, C in (("bn1", 8), ("bn2", 16), ("bn3", 100)):
        p[name + "_rm"] = 0.2 * torch.randn(C, generator=gen)
        p[name + "_rv"] = 0.5 + torch.rand(C, generator=gen)
    return {"N": N, "T": T, "series": series, "p": p, "dg": dg}


def global_ref(dtype, case, training=True, momentum=MOMENTUM, stats_out=None):
    """O.dgl_global_feature under autograd in ``dtype`` with loss sum(g * dg).  -> {"g" [N,100], "grads": the twelve gradients under
    the StepDglParams names (training only), "running": the six running statistics after the call (momentum, unbiased variance;
    unchanged in eval mode)}.  stats_out (dict): receives the oracle's batch statistics name -> (mean, unbiased variance)."""
    p = {global_key(k): v.detach().to(dtype).clone().requires_grad_(k in GLOBAL_TRAINABLE and training) for k, v in case["p"].items()}
    stats = {} if stats_out is None else stats_out
    with torch.set_grad_enabled(training):
        g = O.dgl_global_feature(case["series"].to(dtype).t(), p, EDGE_PRE, training, stats=stats)
    out = {"g": g.detach(), "grads": {}, "running": {}}
    if training:
        (g * case["dg"].to(dtype)).sum().backward()
        out["grads"] = {k: p[global_key(k)].grad for k in GLOBAL_TRAINABLE}
    for bn in ("bn1", "bn2", "bn3"):
        rm, rv = p[global_key(bn + "_rm")].detach(), p[global_key(bn + "_rv")].detach()
        if training:
            mu, var_u = stats[bn]
            rm, rv = (1 - momentum) * rm + momentum * mu, (1 - momentum) * rv + momentum * var_u
        out["running"][bn + "_rm"], out["running"][bn + "_rv"] = rm, rv
    return out


def flat_global(out):
    """every compared tensor of a result of the global branch (device, reference or model) under one name"""
    return {"g": out["g"], **out["grads"], **out["running"]}


def global_bf16_model(case, rounding=True, storage="bf16", training=True, momentum=MOMENTUM):
    """What bf16 mode (StepDglParams.gemm_bf16 = 1) computes, in float64 arithmetic with a round-to-nearest-even bf16 exactly where
    the device rounds -- the forward and the hand-written backward of step_amd/csrc/dgl.hip / dgl_conv_mfma.hip / the fused epilogues
    of gemm_bf16.hip, step by step (this is not autograd of a rounded forward: the device's backward is not that either).  With
    rounding off it is the oracle's function and gradient (tests/test_direct_ref_host.py holds it to global_ref(float64) at 1e-12).

    storage = "bf16" (the default of the mode: channels-last bf16 rows):
      conv1 is f32 arithmetic; its output is STORED rounded (a1), BatchNorm1's sums are taken from the f32 values before that rounding
      (conv1_fwd_cl_kernel).  conv2 multiplies the stored rows by bf16(w * scale1) and adds the folded bias in f32 (conv2_pack_kernel);
      BatchNorm2's sums again come from the f32 values, the output is stored rounded (a2).  The fc multiplies a2 by
      bf16(fc_w * scale2) and starts from the f32 shift term (fc_prep_kernel).  Backward: BatchNorm3 / ReLU in f32; G = bf16(dgpre)^T a2,
      un-permuted with BatchNorm2's affine in f32, BatchNorm2's two sums from fc_w . G and fc_w . colsum in f32 (fc_unpermute_kernel);
      dz2 = the BatchNorm2 backward transform of bf16(dgpre) bf16(fc_w * scale2) with x = the stored a2, stored rounded (the
      GEMM_FUSED_INTERLEAVED epilogue); the conv2 weight-gradient sums and the conv2 bias gradient from the STORED dz2 and a1
      (conv2_wgrad_cl_kernel), normalised afterwards (conv2_wgrad_finish_kernel, raw = 1); dz1 from the stored dz2, bf16(w * scale1)
      and the stored a1, stored rounded (conv2_dgrad_cl_kernel); conv1's gradients from the stored dz1 and bf16(series).
    storage = "f32" (STEP_DGL_F32_STORAGE=1, with the fused BatchNorm backward: T - 18 >= 128): the activations and their gradients
      stay f32 and every product rounds its two operands as it reads them: conv2 bf16(scale1 a1 + shift1) bf16(w); the fc
      bf16(scale2 a2 + shift2) bf16(fc_w); dz2 from bf16(dgpre) bf16(fc_w) with the transform in f32; the conv2 weight gradient
      bf16(dz2) bf16(xhat1) with the bias gradient from the f32 dz2; dz1 from bf16(dz2) bf16(w); conv1's from bf16(dz1) bf16(series)."""
    assert storage in ("bf16", "f32")
    F = torch.nn.functional
    R = round_bf16 if rounding else (lambda t: t)
    cl = storage == "bf16"
    f64 = torch.float64
    P = {k: v.detach().to(f64) for k, v in case["p"].items()}
    x, dg = case["series"].to(f64), case["dg"].to(f64)
    N, T = x.shape
    T1, T2 = T - 9, T - 18
    assert cl or T2 >= 128 or not training
    eps = O.BN_EPS
    ch = lambda v: v.view(1, -1, 1)
    W1, W2, Wf = P["conv1_w"], P["conv2_w"], P["fc_w"].view(100, 16, T2)
    running = {}

    def statistics(a, dims, name):          # mean, 1 / sqrt(var + eps) of the values BEFORE any rounding
        if training:
            n = a.numel() // a.shape[1]
            mu = a.mean(dims)
            var = ((a - (ch(mu) if a.dim() == 3 else mu)) ** 2).mean(dims)
            running[name + "_rm"] = (1 - momentum) * P[name + "_rm"] + momentum * mu
            running[name + "_rv"] = (1 - momentum) * P[name + "_rv"] + momentum * var * (n / max(n - 1, 1))
        else:
            mu, var = P[name + "_rm"], P[name + "_rv"]
            running[name + "_rm"], running[name + "_rv"] = mu, var
        return mu, (var + eps).rsqrt()

    # ---- forward
    c1 = torch.relu(F.conv1d(x.unsqueeze(1), W1, P["conv1_b"]))
    mu1, rstd1 = statistics(c1, (0, 2), "bn1")
    sc1 = P["bn1_w"] * rstd1
    sh1 = P["bn1_b"] - mu1 * sc1
    if cl:
        a1, w2f = R(c1), R(W2 * ch(sc1))
        c2 = torch.relu(F.conv1d(a1, w2f, P["conv2_b"] + (W2.sum(2) * sh1).sum(1)))
    else:
        a1 = c1
        c2 = torch.relu(F.conv1d(R(c1 * ch(sc1) + ch(sh1)), R(W2), P["conv2_b"]))
    mu2, rstd2 = statistics(c2, (0, 2), "bn2")
    sc2 = P["bn2_w"] * rstd2
    sh2 = P["bn2_b"] - mu2 * sc2
    a2 = R(c2)                                    # what the fc weight gradient reads in either storage
    if cl:
        wp = R(Wf * ch(sc2))
        gpre = torch.einsum("nct,oct->no", a2, wp) + (Wf * ch(sh2)).sum((1, 2)) + P["fc_b"]
    else:
        gpre = torch.einsum("nct,oct->no", R(c2 * ch(sc2) + ch(sh2)), R(Wf)) + P["fc_b"]
    r3 = torch.relu(gpre)
    mu3, rstd3 = statistics(r3, (0,), "bn3")
    out = {"g": (r3 - mu3) * rstd3 * P["bn3_w"] + P["bn3_b"], "grads": {}, "running": running}
    if not training:
        return out

    # ---- backward
    gr = out["grads"]
    xh3 = (r3 - mu3) * rstd3
    S1, S2 = dg.sum(0), (dg * xh3).sum(0)
    gr["bn3_w"], gr["bn3_b"] = S2, S1
    dgpre = torch.where(gpre > 0, P["bn3_w"] * rstd3 * (dg - S1 / N - xh3 * S2 / N), torch.zeros_like(dg))
    colsum = dgpre.sum(0)
    gr["fc_b"] = colsum
    G = torch.einsum("no,nct->oct", R(dgpre), a2)
    gr["fc_w"] = (ch(sc2) * G + ch(sh2) * colsum.view(-1, 1, 1)).reshape(100, -1)
    S1 = torch.einsum("oct,o->c", Wf, colsum)
    S2 = rstd2 * ((Wf * G).sum((0, 2)) - mu2 * S1)
    gr["bn2_w"], gr["bn2_b"] = S2, S1
    m1, m2, kc = S1 / (N * T2), S2 / (N * T2), P["bn2_w"] * rstd2
    if cl:
        v = torch.einsum("no,oct->nct", R(dgpre), wp)
        dz2 = R(torch.where(a2 > 0, v - ch(kc * m1) - (a2 - ch(mu2)) * ch(kc * m2 * rstd2), torch.zeros_like(v)))
        dz2_op = dz2
    else:
        v = torch.einsum("no,oct->nct", R(dgpre), R(Wf))
        dz2 = torch.where(c2 > 0, ch(kc) * (v - ch(m1) - (c2 - ch(mu2)) * ch(m2 * rstd2)), torch.zeros_like(v))
        dz2_op = R(dz2)
    db2 = dz2.sum((0, 2))
    corr = lambda inp, dz: F.conv1d(inp.transpose(0, 1), dz.transpose(0, 1)).transpose(0, 1)          # [co, ci, kk] = sum_{n,t} dz[n,co,t] inp[n,ci,t+kk]
    if cl:
        Gp = ch(rstd1) * (corr(a1, dz2_op) - ch(mu1) * db2.view(-1, 1, 1))
    else:
        Gp = corr(R((c1 - ch(mu1)) * ch(rstd1)), dz2_op)
    gr["conv2_w"] = ch(P["bn1_w"]) * Gp + ch(P["bn1_b"]) * db2.view(-1, 1, 1)
    gr["conv2_b"] = db2
    S1 = (W2.sum(2) * db2.view(-1, 1)).sum(0)
    S2 = (W2 * Gp).sum((0, 2))
    gr["bn1_w"], gr["bn1_b"] = S2, S1
    m1, m2, kc = S1 / (N * T1), S2 / (N * T1), P["bn1_w"] * rstd1
    if cl:
        d_a1 = F.conv_transpose1d(dz2_op, w2f)
        dz1 = R(torch.where(a1 > 0, d_a1 - ch(kc * m1) - (a1 - ch(mu1)) * ch(kc * m2 * rstd1), torch.zeros_like(d_a1)))
        dz1_op = dz1
    else:
        d_a1 = F.conv_transpose1d(dz2_op, R(W2))
        dz1 = torch.where(c1 > 0, ch(kc) * (d_a1 - ch(m1) - (c1 - ch(mu1)) * ch(m2 * rstd1)), torch.zeros_like(d_a1))
        dz1_op = R(dz1)
    gr["conv1_w"] = F.conv1d(R(x).unsqueeze(0), dz1_op.transpose(0, 1)).view(8, 1, 10)
    gr["conv1_b"] = dz1.sum((0, 2))
    return out


class _Guarded:
    """n floats for the library between two guard bands of GUARD floats each (a fixed bit pattern in front, another one behind); the
    library is handed exactly the n floats in the middle, which start as NaN bytes"""

    def __init__(self, n, dev):
        self.n = int(n)
        self.raw = torch.empty(self.n + 2 * GUARD, dtype=torch.int32, device=dev)
        self.raw[:GUARD] = _GUARD_FRONT
        self.raw[GUARD + self.n:] = _GUARD_BACK
        self.raw[GUARD:GUARD + self.n] = -1
        self.t = self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def intact(self):
        return bool((self.raw[:GUARD] == _GUARD_FRONT).all()) and bool((self.raw[GUARD + self.n:] == _GUARD_BACK).all())


def _global_buffers(lib, N, T, dev):
    return (_Guarded(lib.step_dgl_global_saved_floats(N, T), dev), _Guarded(lib.step_dgl_global_work_floats(N, T, 0), dev),
            _Guarded(lib.step_dgl_global_work_floats(N, T, 1), dev))


def run_global(case, bf16=0, training=1, momentum=MOMENTUM, grad_fill=None, phases=(0,), fresh_fc=False, buffers=None, backward=True):
    """step_dgl_global_forward + step_dgl_global_backward_phase (once per entry of ``phases``, in the same work buffer) through ctypes.
    saved / work / g and, with fresh_fc, grads.fc_w start as NaN bytes; saved and both work buffers hold exactly
    step_dgl_global_{saved,work}_floats floats between two guard bands.  grad_fill: name -> G0 the gradient buffers start from (None:
    zeros).  buffers: those of an earlier call, to run in again (not refilled).  -> host copies: g, grads (after the last phase),
    grads_after (one dict per phase), running / initial (the six statistics after / before), guards_intact, buffers."""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    dev = torch.device("cuda")
    N, T = case["N"], case["T"]
    lib = L.lib()
    series = case["series"].to(dev).contiguous()
    params = {k: v.to(dev).contiguous().clone() for k, v in case["p"].items()}
    struct = fill_dgl_struct(params, bf16)
    if buffers is None:
        buffers = _global_buffers(lib, N, T, dev)
    saved, wfwd, wbwd = buffers
    g = _nan_floats(N * 100, dev).view(N, 100)
    initial = {k: params[k].cpu() for k in GLOBAL_RUNNING}
    st = L.stream()
    L.call("step_dgl_global_forward", L.ptr(series), N, T, ctypes.byref(struct), int(training), float(momentum), L.ptr(saved.t), L.ptr(wfwd.t),
           L.ptr(g), st)
    torch.cuda.synchronize()
    out = {"g": g.cpu(), "grads": {}, "grads_after": [], "running": {k: params[k].cpu() for k in GLOBAL_RUNNING}, "initial": initial,
           "buffers": buffers}
    if training and backward:
        dg = case["dg"].to(dev).contiguous()
        grads = {k: (torch.zeros_like(params[k]) if grad_fill is None else grad_fill[k].to(dev).contiguous().clone()) for k in GLOBAL_TRAINABLE}
        if fresh_fc:
            grads["fc_w"] = _nan_floats(params["fc_w"].numel(), dev).view_as(params["fc_w"])
        gstruct = fill_dgl_struct(grads, bf16)
        for ph in phases:
            L.call("step_dgl_global_backward_phase", L.ptr(series), N, T, ctypes.byref(struct), L.ptr(saved.t), L.ptr(dg), L.ptr(wbwd.t),
                   ctypes.byref(gstruct), int(ph) | (FRESH_FC_GRAD if fresh_fc else 0), st)
            torch.cuda.synchronize()
            out["grads_after"].append({k: v.cpu() for k, v in grads.items()})
        out["grads"] = out["grads_after"][-1]
    out["guards_intact"] = all(b.intact() for b in buffers)
    return out


def run_global_sliced(case, bounds):
    """The time-sliced entry points step_dgl_global_{forward,backward}_shard in ONE process, without a communicator: this driver is the
    caller of include/step_hip.h.  bounds: [(a, b)] column ranges of the T - 18 conv2 outputs; every slice has its own saved / work
    (guarded, NaN-filled), the series columns [a, b + 18) and the weight columns fc.weight.view(100, 16, T - 18)[:, :, a:b].  Between
    the calls the driver sums over the slices, with torch on the one stream: `sums` [0,16) after forward phase 1 and [16,48) after
    phase 2, gpre after phase 3; the 32 dots (offset item 10) after backward phase 1 and the 1296 graw values (item 11) after phase 3.
    own1 = b - a (+ 9 on the last slice), count1 / count2 = N (T - 9) / N (T - 18) of the whole series.  bf16 mode, fc_w stored
    (STEP_DGL_FRESH_FC_GRAD, as step.py calls it) into NaN bytes.  -> g (asserted identical on every slice), the fc weight gradient
    reassembled from the slices, the conv1 gradients summed over them, the rest from slice 0; running / initial of slice 0."""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    dev = torch.device("cuda")
    N, T = case["N"], case["T"]
    T2 = T - 18
    lib = L.lib()
    st = L.stream()
    dg = case["dg"].to(dev).contiguous()
    assert bounds[0][0] == 0 and bounds[-1][1] == T2 and all(bounds[i][1] == bounds[i + 1][0] for i in range(len(bounds) - 1))
    sl = []
    for i, (a, b) in enumerate(bounds):
        s = {"a": a, "b": b, "Ts": b - a + 18}
        s["series"] = case["series"][:, a:b + 18].contiguous().to(dev)
        s["params"] = {k: v.to(dev).contiguous().clone() for k, v in case["p"].items() if k != "fc_w"}
        s["params"]["fc_w"] = case["p"]["fc_w"].view(100, 16, T2)[:, :, a:b].contiguous().view(100, -1).to(dev)
        s["struct"] = fill_dgl_struct(s["params"], 1)
        s["shard"] = L.StepDglShard()
        s["shard"].own1, s["shard"].count1, s["shard"].count2 = (b - a) + (9 if i == len(bounds) - 1 else 0), float(N) * (T - 9), float(N) * T2
        s["buffers"] = _global_buffers(lib, N, s["Ts"], dev)
        s["sums"] = torch.zeros(48, dtype=torch.float64, device=dev)
        s["g"] = _nan_floats(N * 100, dev).view(N, 100)
        go = lib.step_dgl_global_offset(N, s["Ts"], 2)
        s["gpre"] = s["buffers"][0].t[go:go + N * 100]
        o_dots, o_graw = lib.step_dgl_global_offset(N, s["Ts"], 10), lib.step_dgl_global_offset(N, s["Ts"], 11)
        assert go >= 0 and o_dots >= 0 and o_graw + 1296 <= s["buffers"][2].n
        s["dots"], s["graw"] = s["buffers"][2].t[o_dots:o_dots + 32], s["buffers"][2].t[o_graw:o_graw + 1296]
        s["grads"] = {k: torch.zeros_like(v) for k, v in s["params"].items() if k in GLOBAL_TRAINABLE and k != "fc_w"}
        s["grads"]["fc_w"] = _nan_floats(s["params"]["fc_w"].numel(), dev).view_as(s["params"]["fc_w"])
        s["gstruct"] = fill_dgl_struct(s["grads"], 1)
        sl.append(s)
    initial = {k: sl[0]["params"][k].cpu() for k in GLOBAL_RUNNING}

    def sum_over_slices(views):
        total = torch.stack(views).sum(0)
        for v in views:
            v.copy_(total)

    for phase in (1, 2, 3, 4):
        for s in sl:
            L.call("step_dgl_global_forward_shard", L.ptr(s["series"]), N, s["Ts"], ctypes.byref(s["struct"]), 1, MOMENTUM, L.ptr(s["buffers"][0].t),
                   L.ptr(s["buffers"][1].t), L.ptr(s["sums"]), L.ptr(s["g"]), ctypes.byref(s["shard"]), phase, st)
        if phase == 1:
            sum_over_slices([s["sums"][:16] for s in sl])
        elif phase == 2:
            sum_over_slices([s["sums"][16:] for s in sl])
        elif phase == 3:
            sum_over_slices([s["gpre"] for s in sl])
    for phase in (1, 3, 4):
        for s in sl:
            L.call("step_dgl_global_backward_shard", L.ptr(s["series"]), N, s["Ts"], ctypes.byref(s["struct"]), L.ptr(s["buffers"][0].t), L.ptr(dg),
                   L.ptr(s["buffers"][2].t), ctypes.byref(s["gstruct"]), ctypes.byref(s["shard"]), phase | FRESH_FC_GRAD, st)
        if phase == 1:
            sum_over_slices([s["dots"] for s in sl])
        elif phase == 3:
            sum_over_slices([s["graw"] for s in sl])
    torch.cuda.synchronize()
    for s in sl[1:]:
        assert torch.equal(s["g"], sl[0]["g"]), "g differs between the slices"
    grads = {k: v.cpu() for k, v in sl[0]["grads"].items()}
    grads["fc_w"] = torch.cat([s["grads"]["fc_w"].view(100, 16, -1) for s in sl], dim=2).reshape(100, -1).cpu()
    for k in ("conv1_w", "conv1_b"):
        grads[k] = torch.stack([s["grads"][k] for s in sl]).sum(0).cpu()
    return {"g": sl[0]["g"].cpu(), "grads": grads, "running": {k: sl[0]["params"][k].cpu() for k in GLOBAL_RUNNING}, "initial": initial,
            "guards_intact": all(b.intact() for s in sl for b in s["buffers"])}


@functools.lru_cache(maxsize=None)
def cached_global_case(N, T):
    return global_case(N, T)


@functools.lru_cache(maxsize=None)
def cached_global_ref(N, T, dtype, training=True, momentum=MOMENTUM):
    return global_ref(dtype, cached_global_case(N, T), training=training, momentum=momentum)


@functools.lru_cache(maxsize=None)
def cached_global_model(N, T, storage="bf16", training=True):
    return global_bf16_model(cached_global_case(N, T), storage=storage, training=training)
