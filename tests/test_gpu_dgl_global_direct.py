"""The graph learner's global-feature kernels (step_amd/csrc/dgl.hip, dgl_conv_mfma.hip: conv1 -> BatchNorm1 -> conv2 -> BatchNorm2 -> fc
-> BatchNorm3 on the whole training series) called directly and held to a float64 reference.

``step_dgl_global_forward`` + ``step_dgl_global_backward_phase`` (and the time-sliced ``*_shard`` entry points) run through ctypes
(tests/direct_ref.py), outside ``step_amd.STEP``, and every result -- g, the twelve gradients, the six running statistics, which start
off 0 / 1 -- is compared with ``oracle/step_oracle.py`` in float64.  The shapes (direct_ref.GLOBAL_SHAPES) sit on the kernels' edges:
T - 18 = 1 and 10 (one kernel width), 127 / 128 (three-pass / fused BatchNorm2 backward in f32 mode), 256 (WG_SC), 1024 / 1025
(FW_TT), 3584 / 3585 (WG_SC x WG_PASSES), row-tile tails of the fc GEMMs (N = 70, 131, 260), and 8200 nodes x 40 steps (forward only:
float32 autograd on the CPU is itself 1e-3 off there) for the sliced f64-atomic statistics of dgl_bn_stats (nblk >= 8192).  saved and
both work buffers hold exactly step_dgl_global_{saved,work}_floats floats of NaN bytes between two guard bands.

Tolerance, the rule of tests/test_gpu_gwnet_direct.py: e_dev = err(device, f64) <= M * e_f32 + FLOOR with e_f32 = err(f32 oracle, f64),
err = relative L2 (no tensor of this branch is zero in exact arithmetic: a ReLU stands between every bias and the next BatchNorm).
FLOOR = the largest difference between two runs in fresh buffers (test_buffers_can_be_reused), rounded up to two digits.
tests/test_direct_ref_host.py asserts for every tensor of every shape that M * e_f32 + FLOOR <= 1e-4 (the tightest fixed bound this
rule supersedes: g < 1e-4, gradients < 2e-3 in tests/test_gpu_dgl_conv.py) and that the inputs are well conditioned (no BatchNorm
variance below 1e-3, e_f32 <= 2e-5).  bf16 mode: e_dev <= 2 * e_model + the f32 bound for EVERY tensor, e_model = error of
direct_ref.global_bf16_model against float64.

Measured on an MI355X (also in DESIGN.md section 2):
  f32 mode, e_dev / e_f32 over 465 compared tensors: largest 2.92 (conv1_b at (13, 1042): e_dev 3.67e-6, e_f32 1.26e-6), then 2.54
  (bn1_b at (260, 150)), 2.05, 2.04, 1.99; everything else below 2.  The largest e_dev at all is 9.3e-6 (bn1_b at (13, 3603), ratio
  1.36).  The backbone's rule -- 4 x the largest ratio, rounded up to a power of two -- gives 16, and 16 does not meet the condition
  above: bn1_b has e_f32 = 8.24e-6 at (70, 600) and 6.70e-6 at (13, 3603), where 16 * e_f32 + FLOOR = 1.35e-4 / 1.10e-4.  No kernel is
  behind that: the device is at ratio 1.1 - 1.4 on exactly those tensors, and the ratios near 3 belong to gradients whose e_dev
  (3.7e-6, 4.7e-6) is barely above the run-to-run noise of the f32 atomics that sum them (conv_bwd_weight_kernel: one atomicAdd per
  node).  M is therefore NOT raised to 16 but set to the largest power of two that keeps every bound at or below 1e-4:  M = 8, 2.7 x
  the largest measured ratio (largest bound: 6.9e-5, bn1_b at (70, 600)).
  run-to-run noise (two runs in fresh buffers): 2.97e-6 (conv1_b at (131, 300)), 1.42e-6 (conv2_b at (13, 3603)) -> FLOOR = 3.0e-6.
  bf16 mode: device / model between 0.98 and 1.02 on every tensor with a non-zero model error, over all fourteen shapes, the two-phase
  and the sliced cases (largest: 1.02, bn1_b at (33, 28): device 9.63e-2, model 9.48e-2 from float64; g at (13, 1043): 7.9e-3 both).
  The four cancelling sums conv1_b / conv2_b / bn1_b / bn2_b need no larger factor than 2: the model reproduces the device's rounding,
  not another draw of it.  The f32-storage variant is held to the model's own switch for it (storage="f32"), same agreement.
  Shapes: bf16 mode accepts every shape down to T - 18 = 1; nothing is rejected (the only bound, >= 128 columns per time slice in
  step_dgl_global_backward_shard, is pinned by test_short_time_slice_is_rejected_before_any_launch).
  Time slices against the unsliced bf16 run (four cases): g 2e-7 .. 1.9e-5, fc_w 1e-7 .. 3.6e-4, the conv gradients up to 2.9e-3 (conv1_w).
"""
import pytest
import torch

from tests import direct_ref as D

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SHAPES, FORWARD_ONLY, SLICED = D.GLOBAL_SHAPES, D.GLOBAL_FORWARD_ONLY, D.GLOBAL_SLICED
M, FLOOR = D.GLOBAL_M, D.GLOBAL_FLOOR
# M: see the docstring -- the largest power of two with M * e_f32 + FLOOR <= 1e-4 everywhere, 2.7 x the largest measured ratio
FC_SIDE = ("fc_w", "fc_b", "bn3_w", "bn3_b")          # what backward phase 1 finishes


def _refs(N, T, **kw):
    return D.cached_global_ref(N, T, F64, **kw), D.cached_global_ref(N, T, F32, **kw)


def _held(tag, dev, r64, r32, model=None, minus=None, only=None):
    """every tensor of the device result (or those in ``only``) against float64 under the f32 rule, or -- with a model -- the bf16 rule;
    minus: name -> G0 subtracted first (the `+=` contract).  Guard bands intact, everything finite (Compare.add)."""
    fd, f64, f32 = D.flat_global(dev), D.flat_global(r64), D.flat_global(r32)
    assert set(fd) == set(f64), (sorted(fd), sorted(f64))
    fm = None if model is None else D.flat_global(model)
    cmp_ = D.Compare(tag, M, FLOOR, FLOOR)
    for k in fd:
        if only is not None and k not in only:
            continue
        x = fd[k].double() - minus[k].double() if (minus is not None and k in minus) else fd[k]
        extra = 0.0
        if fm is not None:
            e_model = D.rel_l2(fm[k], f64[k])
            extra = 2 * e_model
            e_dev = D.rel_l2(x, f64[k])
            print(f"MODEL {tag} {k:<8s} e_dev={e_dev:.3e} e_model={e_model:.3e} dev/model={e_dev / e_model if e_model > 0 else float('nan'):6.2f}")
        cmp_.add(k, x, f64[k], f32[k], extra=extra)
    assert dev["guards_intact"], f"{tag}: a guard band behind or in front of saved / work was written"
    cmp_.finish()


def _model(N, T, **kw):
    return D.cached_global_model(N, T, **kw)


# ----------------------------------------------------------------------------------------- f32 mode
@pytest.mark.parametrize("N,T", SHAPES)
def test_f32_training_matches_float64(N, T):
    _held(f"f32 N={N} T={T}", D.run_global(D.cached_global_case(N, T)), *_refs(N, T))


@pytest.mark.parametrize("N,T", FORWARD_ONLY)
@pytest.mark.parametrize("bf16", [0, 1])
def test_many_partial_rows_forward(N, T, bf16):
    """nblk >= 8192: BatchNorm1 / BatchNorm2 statistics through bn_sums_sliced_kernel (f64 atomics); g and the six running statistics"""
    c = D.cached_global_case(N, T)
    r64, r32 = (dict(r, grads={}) for r in _refs(N, T))          # (the cached references are shared: copies without the gradients)
    model = dict(_model(N, T), grads={}) if bf16 else None
    _held(f"forward bf16={bf16} N={N} T={T}", D.run_global(c, bf16=bf16, backward=False), r64, r32, model=model)


# ----------------------------------------------------------------------------------------- bf16 mode
@pytest.mark.parametrize("N,T", SHAPES)
def test_bf16_training_within_the_operand_model(N, T):
    """every shape: the mode's kernels have no lower bound on T - 18 (the interleaved epilogue needs channels % 8 == 0 and 16-byte
    aligned rows, which 16 channels of bf16 always give), so nothing is rejected"""
    _held(f"bf16 N={N} T={T}", D.run_global(D.cached_global_case(N, T), bf16=1), *_refs(N, T), model=_model(N, T))


# ----------------------------------------------------------------------------------------- eval mode, momentum
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("N,T", [(33, 28), (13, 1043), (131, 300)])
def test_eval_mode(N, T, bf16):
    """training = 0: g from the running statistics (which are off 0 / 1), and those are bit-unchanged afterwards"""
    dev = D.run_global(D.cached_global_case(N, T), bf16=bf16, training=0)
    r64, r32 = _refs(N, T, training=False)
    _held(f"eval bf16={bf16} N={N} T={T}", dev, r64, r32, model=_model(N, T, training=False) if bf16 else None)
    for k, v in dev["initial"].items():
        assert torch.equal(dev["running"][k], v), k
    assert D.rel_l2(dev["g"], D.cached_global_ref(N, T, F64)["g"]) > 1e-2          # (not the batch statistics)


def test_momentum():
    N, T = 13, 146
    dev = D.run_global(D.cached_global_case(N, T), momentum=0.3)
    _held(f"momentum=0.3 N={N} T={T}", dev, *_refs(N, T, momentum=0.3))
    r01 = D.cached_global_ref(N, T, F64)["running"]
    for k in D.GLOBAL_RUNNING:          # (momentum 0.1 is another result)
        assert D.rel_l2(dev["running"][k], r01[k]) > 1e-3, k


# ----------------------------------------------------------------------------------------- the gradient struct's contract
def _g0(r64, seed=5):
    g = torch.Generator().manual_seed(seed)
    # G0 of each tensor's own scale (half its RMS): the rounding of the sum then stays at float32 precision of the gradient itself
    return {k: (torch.randn(v.shape, generator=g) * max(0.5 * float(v.double().pow(2).mean().sqrt()), 1e-12)).float() for k, v in r64["grads"].items()}


@pytest.mark.parametrize("fresh_fc", [False, True])
@pytest.mark.parametrize("N,T", [(13, 146), (70, 300)])
def test_backward_accumulates_into_the_gradients(N, T, fresh_fc):
    """`+=`: gradient buffers that start at G0 end at G0 + gradient.  With STEP_DGL_FRESH_FC_GRAD grads.fc_w starts as NaN bytes and
    ends finite and within bounds (stored); the other eleven still accumulate."""
    r64, r32 = _refs(N, T)
    G0 = _g0(r64)
    dev = D.run_global(D.cached_global_case(N, T), grad_fill=G0, fresh_fc=fresh_fc)
    for k, v in G0.items():
        assert not torch.equal(dev["grads"][k], v), k
    minus = {k: v for k, v in G0.items() if not (fresh_fc and k == "fc_w")}
    _held(f"accumulate fresh_fc={fresh_fc} N={N} T={T}", dev, r64, r32, minus=minus)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("N,T", [(13, 1043), (131, 300)])
def test_two_phase_backward(N, T, bf16):
    """phase 1, then phase 2 in the same work buffer, as step.py calls it: after phase 1 alone fc_w / fc_b / bn3_w / bn3_b are finished
    and the other eight untouched (bit-equal to their G0); after phase 2 all twelve are within bounds"""
    r64, r32 = _refs(N, T)
    G0 = _g0(r64, seed=6)
    dev = D.run_global(D.cached_global_case(N, T), bf16=bf16, grad_fill=G0, phases=(1, 2))
    model = _model(N, T) if bf16 else None
    first = dict(dev, grads=dev["grads_after"][0])
    for k in D.GLOBAL_TRAINABLE:
        if k not in FC_SIDE:
            assert torch.equal(first["grads"][k], G0[k]), f"{k} written by phase 1"
    _held(f"phase 1 bf16={bf16} N={N} T={T}", first, r64, r32, model=model, minus=G0, only=FC_SIDE)
    _held(f"phase 1+2 bf16={bf16} N={N} T={T}", dev, r64, r32, model=model, minus=G0)


@pytest.mark.parametrize("N,T", [(131, 300), (13, 3603)])
def test_buffers_can_be_reused(N, T):
    """a second forward + backward in the same saved / work buffers is as good as the first (held to the reference), and no further
    from a run in fresh buffers than four times the difference of two such runs plus the floor -- which this test measures"""
    c = D.cached_global_case(N, T)
    r64, r32 = _refs(N, T)
    a, b = D.run_global(c), D.run_global(c)
    again = D.run_global(c, buffers=D.run_global(c)["buffers"])
    _held(f"reuse N={N} T={T}", again, r64, r32)
    fa, fb, fx = D.flat_global(a), D.flat_global(b), D.flat_global(again)
    worst, bad = 0.0, []
    for k in fa:
        noise, reuse = D.rel_l2(fb[k], fa[k]), D.rel_l2(fx[k], fa[k])
        worst = max(worst, noise)
        if noise > 0 or reuse > 0:
            print(f"NOISE N={N} T={T} {k:<8s} fresh-vs-fresh {noise:.3e} reuse-vs-fresh {reuse:.3e}")
        if not reuse <= 4 * noise + FLOOR:
            bad.append((k, noise, reuse))
    print(f"NOISE N={N} T={T} worst fresh-vs-fresh rel_l2 {worst:.3e}")
    assert not bad, bad


# ----------------------------------------------------------------------------------------- time slices
@pytest.mark.parametrize("N,T,bounds", SLICED)
def test_time_slices(N, T, bounds):
    """step_dgl_global_{forward,backward}_shard with this test as the caller that sums between the phases: held to float64 under the
    bf16 rule; the difference to the unsliced bf16 run is printed"""
    c = D.cached_global_case(N, T)
    dev = D.run_global_sliced(c, bounds)
    _held(f"sliced N={N} T={T} {bounds}", dev, *_refs(N, T), model=_model(N, T))
    whole = D.flat_global(D.run_global(c, bf16=1))
    for k, v in D.flat_global(dev).items():
        print(f"SLICED N={N} T={T} {len(bounds)} slices {k:<8s} rel_l2 to the unsliced bf16 run {D.rel_l2(v, whole[k]):.3e}")


# ----------------------------------------------------------------------------------------- the two environment variants
def test_f32_storage_variant(monkeypatch):
    """bf16 mode with STEP_DGL_F32_STORAGE=1 (read per call): [N][C][T] f32 activations, operands rounded as each product reads them --
    held to the bf16 rule with the model's switch for that variant (storage="f32")"""
    N, T = 13, 1043
    monkeypatch.setenv("STEP_DGL_F32_STORAGE", "1")
    dev = D.run_global(D.cached_global_case(N, T), bf16=1)
    _held(f"bf16 f32-storage N={N} T={T}", dev, *_refs(N, T), model=_model(N, T, storage="f32"))


def test_legacy_batchnorm_backward_variant(monkeypatch):
    """f32 mode with STEP_DGL_LEGACY_BN=1 (read per call): the three-pass BatchNorm2 backward at T - 18 >= 128, held to the f32 rule"""
    N, T = 13, 1043
    monkeypatch.setenv("STEP_DGL_LEGACY_BN", "1")
    _held(f"f32 legacy-bn N={N} T={T}", D.run_global(D.cached_global_case(N, T)), *_refs(N, T))


def test_short_time_slice_is_rejected_before_any_launch():
    """the one shape bound of the mode (include/step_hip.h): a slice of fewer than 128 conv2 columns in the time-sliced backward is
    refused with STEP_ERR_ARG and a message, and nothing was launched: the gradient and work buffers keep their bytes"""
    import ctypes
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    N, Ts = 13, 18 + 127
    c = D.global_case(N, Ts)
    dev = torch.device("cuda")
    lib = L.lib()
    params = {k: v.to(dev).contiguous() for k, v in c["p"].items()}
    grads = {k: torch.full_like(params[k], 7.0) for k in D.GLOBAL_TRAINABLE}
    saved, _, work = D._global_buffers(lib, N, Ts, dev)
    shard = L.StepDglShard()
    shard.own1, shard.count1, shard.count2 = 127, float(N) * 300, float(N) * 291
    struct, gstruct = fill_dgl_struct(params, 1), fill_dgl_struct(grads, 1)
    series, dg = c["series"].to(dev).contiguous(), c["dg"].to(dev).contiguous()
    for phase in (1, 3, 4):
        rc = lib.step_dgl_global_backward_shard(L.ptr(series), N, Ts, ctypes.byref(struct), L.ptr(saved.t), L.ptr(dg), L.ptr(work.t),
                                                ctypes.byref(gstruct), ctypes.byref(shard), phase, L.stream())
        assert rc == 1, rc                                  # STEP_ERR_ARG
        assert b"128" in lib.step_last_error()
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in grads.values())
    assert bool((work.raw[D.GUARD:D.GUARD + work.n] == -1).all()) and work.intact() and saved.intact()
