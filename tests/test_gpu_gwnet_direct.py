"""GraphWaveNet backbone kernels (step_amd/csrc/gwnet.hip) called directly and held to a float64 reference.

``step_gwnet_forward`` + ``step_gwnet_backward`` run through ctypes (tests/direct_ref.py), outside ``step_amd.STEP``, at shapes chosen
for a tail each, and every result -- prediction and adjacency gradient (whole and per sample), every gradient of
``trainable_native()``, the running statistics of bn.0 .. bn.6 -- is compared with ``oracle/step_oracle.py`` in float64.

Tolerance (no bound fixed in advance): e_dev = err(device, f64) <= M * e_f32 + FLOOR, where e_f32 = err(f32 oracle, f64) is the same
restatement in the precision the kernels claim; err is the relative L2 norm, or the max-abs difference for the gradients that are zero
in exact arithmetic (gcn biases in front of a train-mode BatchNorm).  M = 4 x the largest ratio measured on the first run, rounded up
to a power of two (the factor covers the device's fast exp / tanh and another summation order); FLOOR = the run-to-run noise of the
atomics measured by the buffer-reuse case.  bf16 mode: e_dev <= 2 * e_model + the f32 bound, e_model = error of the bf16 operand
model against float64.

Measured on an MI355X (also in DESIGN.md section 2):
  f32 mode, e_dev / e_f32 per tensor: largest 3.67 (nodevec2) and 3.60 (nodevec1) at (B, N) = (1, 2); at the other six shapes the
  largest is 2.0 - 2.4, eval mode 1.4 - 1.7, dropout / weighted / `+=` / streams the same.  No ratio above 16.  M = 16.
  run-to-run noise of the atomics (two runs in fresh buffers): 1.78e-6 relative L2 (start_b at (2, 260)), 1.71e-6 max-abs on the
  analytically zero gcn biases -> FLOOR = FLOOR_ABS = 1.8e-6.
  bf16 mode: gemm_bf16 = 1 puts EVERY contraction of gwnet.hip on the bf16 matrix cores, not only the hops, so the hop-only operand
  model is not a model of that mode: at (8, 33) the device is 3.7e-3 (pred) / 6.3e-2 (dadj) / 4-10e-2 (gradients) from float64, the
  hop-only model 2.3e-4 / 1.8e-2 / 1-2e-2.  The model of all of the mode's contractions (direct_ref._RoundedContractions) gives
  3.67e-3 / 6.2e-2 / 4-10e-2 and 6.97e-5 on bn_rm.0 where the device has 6.97e-5: the bf16 cases are bounded by that model; the
  hop-only model bounds the difference between the two operand paths of the hop (last test).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import direct_ref as D

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SHAPES = [(1, 2), (3, 13), (8, 33), (2, 64), (4, 70), (5, 131), (2, 260)]
M = 16.0                                              # 4 x 3.67 (nodevec2 at B = 1, N = 2), rounded up to a power of two
FLOOR, FLOOR_ABS = D.FLOOR_REL, D.FLOOR_ABS           # relative L2; max-abs of the analytically zero gradients


def _zero_keys(f64):
    return [k for k in f64 if float(f64[k].abs().max()) <= D.Compare.ZERO]


def _bf16_compare(tag, fd, f64, f32, fm):
    """bf16 mode: e_dev <= 2 * e_model + the f32 bound per tensor.  The analytically zero gcn-bias gradients are in this mode nothing
    but the rounding noise of a sum of bf16-rounded values (StepGemm.a_rowsum), and the model's value is ANOTHER draw of that noise, not
    its size: per layer the larger of two independent draws' maxima over 32 channels exceeds twice the other now and then (measured:
    device / model between 0.4 and 2.5 over 42 tensors).  They are therefore printed per layer and held to the rule as ONE tensor (the
    seven layers' 224 values: device / model at most 1.8 in the six measured cases)."""
    cmp_ = D.Compare(tag, M, FLOOR, FLOOR_ABS)
    zero = _zero_keys(f64)
    for k in fd:
        cmp_.add(k, fd[k], f64[k], f32[k], extra=2 * D.rel_l2(fm[k], f64[k]), extra_abs=2 * D.max_abs(fm[k], f64[k]), report_only=k in zero)
    if zero:
        cat = lambda f: torch.cat([f[k].double().flatten() for k in zero])
        cmp_.add("zero biases", cat(fd), cat(f64), cat(f32), extra_abs=2 * D.max_abs(cat(fm), cat(f64)))
    return cmp_


def _held_to_reference(tag, dev, r64, r32, model=None, minus=None):
    fd, f64, f32 = D.flat_gwnet(dev), D.flat_gwnet(r64), D.flat_gwnet(r32)
    assert set(fd) == set(f64)
    if model is not None:
        _bf16_compare(tag, fd, f64, f32, D.flat_gwnet(model)).finish()
        return
    cmp_ = D.Compare(tag, M, FLOOR, FLOOR_ABS)
    for k in fd:
        x = fd[k].double() - minus[k].double() if (minus is not None and k in minus) else fd[k]
        cmp_.add(k, x, f64[k], f32[k])
    cmp_.finish()


def _refs(B, N, **kw):
    return D.cached_gwnet_ref(B, N, F64, **kw), D.cached_gwnet_ref(B, N, F32, **kw)


@pytest.mark.parametrize("B,N", SHAPES)
def test_f32_training_matches_float64(B, N):
    dev = D.run_gwnet(D.cached_gwnet_case(B, N))
    _held_to_reference(f"train B={B} N={N}", dev, *_refs(B, N))
    for k in ("bn_rm.7", "bn_rv.7"):          # the dead layer's statistics are not touched without training bit 1
        assert torch.equal(dev["running"][k], dev["initial"][k])


def test_weighted_adjacency_with_diagonal():
    """non-negative real weights and a non-zero diagonal: the + I of both random-walk normalisations and their backward"""
    B, N = 4, 70
    dev = D.run_gwnet(D.cached_gwnet_case(B, N, True))
    _held_to_reference(f"weighted B={B} N={N}", dev, *_refs(B, N, weighted=True))


@pytest.mark.parametrize("B,N", [(3, 13), (4, 70), (2, 260)])
def test_eval_mode(B, N):
    dev = D.run_gwnet(D.cached_gwnet_case(B, N), training=0, backward=False)
    r64, r32 = _refs(B, N, training=False)
    cmp_ = D.Compare(f"eval B={B} N={N}", M, FLOOR, FLOOR_ABS)
    cmp_.add("pred", dev["pred"], r64["pred"], r32["pred"])
    for b in range(B):
        cmp_.add(f"pred[{b}]", dev["pred"][b], r64["pred"][b], r32["pred"][b])
    cmp_.finish()
    for k, v in dev["initial"].items():
        assert torch.equal(dev["running"][k], v), k


@pytest.mark.parametrize("B,N", [(3, 13), (8, 33)])
def test_third_input_channel_is_never_read(B, N):
    """Cin = 3 with channel 2 full of NaN gives what Cin = 2 gives.  Bitwise for everything the forward produces (the prediction, the
    running statistics: no float32 atomics there).  The backward sums with float32 atomics, so two Cin = 2 runs already differ in the
    last bits: its results are finite and within the run-to-run noise of a Cin = 2 run (four times the difference of two such runs,
    plus the suite's floor -- two runs that happen to agree bitwise say nothing about a third)."""
    c = D.cached_gwnet_case(B, N)
    a, a2 = D.flat_gwnet(D.run_gwnet(c)), D.flat_gwnet(D.run_gwnet(c))
    hist3 = torch.cat([c["hist"], torch.full((B, 12, N, 1), float("nan"))], dim=3)
    x = D.flat_gwnet(D.run_gwnet(c, hist=hist3))
    zero = _zero_keys(D.flat_gwnet(D.cached_gwnet_ref(B, N, F64)))
    bitwise = 0
    for k in a:
        assert bool(torch.isfinite(x[k]).all()), k
        bitwise += int(torch.equal(x[k], a[k]))
        if k.startswith(("pred", "bn_r")):
            assert torch.equal(x[k], a[k]), k
        elif k in zero:
            assert D.max_abs(x[k], a[k]) <= 4 * D.max_abs(a2[k], a[k]) + FLOOR_ABS, k
        else:
            assert D.rel_l2(x[k], a[k]) <= 4 * D.rel_l2(a2[k], a[k]) + FLOOR, k
    print(f"Cin=3 B={B} N={N}: {bitwise} of {len(a)} tensors bitwise")


@pytest.mark.parametrize("B,N", [(3, 13), (4, 70)])
def test_dropout_masks_replayed_in_the_reference(B, N):
    c = D.cached_gwnet_case(B, N)
    dev = D.run_gwnet(c, dropout_p=0.3)
    scale = float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    kept = total = 0
    for i, m in enumerate(dev["masks"]):
        assert tuple(m.shape) == (B, 32, N, D.TOUT[i])
        assert bool(((m == 0) | (m == scale)).all()), i
        kept, total = kept + int((m != 0).sum()), total + m.numel()
    sigma = (0.7 * 0.3 / total) ** 0.5
    print(f"dropout B={B} N={N}: keep rate {kept / total:.5f} of {total}, {abs(kept / total - 0.7) / sigma:.2f} sigma from 0.7")
    assert abs(kept / total - 0.7) <= 5 * sigma
    args = (c["sd"], c["hist"], c["last"], c["adj"], c["dpred"])
    r64, r32 = D.gwnet_ref(F64, *args, drop_masks=dev["masks"]), D.gwnet_ref(F32, *args, drop_masks=dev["masks"])
    _held_to_reference(f"dropout B={B} N={N}", dev, r64, r32)
    # the masks matter: the mask-free reference is a different function
    assert D.rel_l2(dev["pred"], D.cached_gwnet_ref(B, N, F64)["pred"]) > 1e-2


@pytest.mark.parametrize("B,N", [(3, 13), (5, 131)])
def test_backward_accumulates_into_the_gradients(B, N):
    """the `+=` contract: gradient buffers that start at G0 end at G0 + gradient; dadj starts as NaN and is stored everywhere"""
    r64, r32 = _refs(B, N)
    g = torch.Generator().manual_seed(5)
    # G0 of each tensor's own scale (half its RMS): the rounding of the sum then stays at float32 precision of the gradient itself
    G0 = {k: (torch.randn(v.shape, generator=g) * max(0.5 * float(v.double().pow(2).mean().sqrt()), 1e-12)).float() for k, v in r64["grads"].items()}
    dev = D.run_gwnet(D.cached_gwnet_case(B, N), grad_fill=G0)
    for k, v in G0.items():
        assert not torch.equal(dev["grads"][k], v), k
    _held_to_reference(f"accumulate B={B} N={N}", dev, r64, r32, minus=G0)


@pytest.mark.parametrize("B,N", [(8, 33), (2, 260)])
def test_buffers_can_be_reused(B, N):
    """a second forward + backward in the same saved / work buffers gives what fresh buffers give, within the run-to-run noise of the
    atomics -- measured as the difference of two runs in fresh buffers (and bounded by four times that, plus the suite's floor)"""
    c = D.cached_gwnet_case(B, N)
    a, b = D.flat_gwnet(D.run_gwnet(c)), D.flat_gwnet(D.run_gwnet(c))
    again = D.flat_gwnet(D.run_gwnet(c, repeat=2))
    r64 = D.flat_gwnet(D.cached_gwnet_ref(B, N, F64))
    worst_rel = worst_abs = 0.0
    bad = []
    for k in a:
        zero = float(r64[k].abs().max()) <= D.Compare.ZERO
        err = D.max_abs if zero else D.rel_l2
        noise, reuse = err(b[k], a[k]), err(again[k], a[k])
        if zero:
            worst_abs = max(worst_abs, noise)
        else:
            worst_rel = max(worst_rel, noise)
        if noise > 0 or reuse > 0:
            print(f"NOISE B={B} N={N} {k:<14s} {'maxabs' if zero else 'rel_l2'} fresh-vs-fresh {noise:.3e} reuse-vs-fresh {reuse:.3e}")
        if not reuse <= 4 * noise + (FLOOR_ABS if zero else FLOOR):
            bad.append((k, noise, reuse))
    print(f"NOISE B={B} N={N} worst fresh-vs-fresh: rel_l2 {worst_rel:.3e}, maxabs of the zero gradients {worst_abs:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("B,N", [(8, 33), (5, 131)])
def test_auxiliary_streams(B, N):
    """aux_stream / leaf_stream NULL and two other streams of the device (joined before reading, as step.py joins them)"""
    c = D.cached_gwnet_case(B, N)
    r64, r32 = _refs(B, N)
    _held_to_reference(f"streams=NULL B={B} N={N}", D.run_gwnet(c), r64, r32)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _held_to_reference(f"streams=aux,leaf B={B} N={N}", D.run_gwnet(c, streams=(s1, s2)), r64, r32)
    _held_to_reference(f"streams=aux B={B} N={N}", D.run_gwnet(c, streams=(s1, None)), r64, r32)


BF16_SHAPES = [(8, 33), (4, 70), (5, 131)]


@pytest.mark.parametrize("B,N", BF16_SHAPES)
def test_bf16_mode_within_the_operand_model(B, N):
    r64, r32 = _refs(B, N)
    _held_to_reference(f"bf16 B={B} N={N}", D.run_gwnet(D.cached_gwnet_case(B, N), bf16=1), r64, r32, model=D.cached_gwnet_ref(B, N, F64, hop="bf16_all"))


XT_SHAPES = [(3, 70), (4, 131), (8, 33)]
_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from tests import direct_ref as D
out = {}
for B, N in %r:
    for k, v in D.flat_gwnet(D.run_gwnet(D.cached_gwnet_case(B, N), bf16=1)).items():
        out[f"{B}_{N}|{k}"] = v.numpy()
np.savez(sys.argv[1], **out)
"""


def test_transposed_hop_operand_with_more_than_one_sample():
    """slots_to_bf16T_kernel + the two-level batch strides of the transposed-operand hop at B > 1.  The threshold (N >= 768) is read
    once per process, so ONE fresh child runs bf16 mode with STEP_HOP_XT_MIN_N=1; its results are held to the reference under the bf16
    bound and to this process's run of the in-place operand path: both round the same operands, so they differ by far less (a quarter
    at most, plus the atomics' floor) than the error of the hops' operand model."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "xt.npz")
        subprocess.run([sys.executable, "-c", _CHILD % (root, XT_SHAPES), path], check=True, env=dict(os.environ, STEP_HOP_XT_MIN_N="1"),
                       cwd=root, timeout=300)
        child = dict(np.load(path))
    failures = []
    for B, N in XT_SHAPES:
        r64, r32, model = D.cached_gwnet_ref(B, N, F64), D.cached_gwnet_ref(B, N, F32), D.cached_gwnet_ref(B, N, F64, hop="bf16_all")
        f64, f32, fall = D.flat_gwnet(r64), D.flat_gwnet(r32), D.flat_gwnet(model)
        fm = D.flat_gwnet(D.cached_gwnet_ref(B, N, F64, hop="bf16"))          # the hops alone: what the two operand paths have in common
        here = D.flat_gwnet(D.run_gwnet(D.cached_gwnet_case(B, N), bf16=1))
        there = {k: torch.from_numpy(child[f"{B}_{N}|{k}"]) for k in f64}
        cmp_ = _bf16_compare(f"xT child B={B} N={N}", there, f64, f32, fall)
        zeros = _zero_keys(f64)
        noise = max(D.max_abs(fall[k], f64[k]) for k in zeros)          # the size of the zero biases' rounding noise in bf16 mode (_bf16_compare)
        worst = 0.0
        for k in f64:
            x = there[k]
            zero = k in zeros
            # (relative figures on the float64 values' scale, so that both terms of the comparison share a denominator)
            diff = D.max_abs(x, here[k]) if zero else float((x.double() - here[k].double()).norm() / (f64[k].norm() + 1e-300))
            e_model = noise if zero else D.rel_l2(fm[k], f64[k])
            floor = FLOOR_ABS if zero else FLOOR
            if e_model > 100 * floor:          # (the ratio means something where the hops' rounding reaches the tensor at all)
                worst = max(worst, diff / e_model)
            if not diff <= 0.25 * e_model + floor:
                failures.append((B, N, k, diff, e_model))
        print(f"XT B={B} N={N}: largest (transposed - in place) / e_model = {worst:.4f}")
        try:
            cmp_.finish()
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures
