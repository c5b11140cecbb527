"""The channels-last kernels of the graph learner's global branch whose BatchNorm / bias sums are reduced per workgroup through LDS and
one in-register wave sum (wave_sum_fast of step_amd/csrc/common.h): conv1_fwd_cl_kernel (runs of 8 steps per lane, 4096 steps per
workgroup), fc_unpermute_kernel (256 steps of one fc row per workgroup), the epilogues of conv2_fwd_cl / conv2_wgrad_cl / conv1_wgrad_cl.
Driven through step_dgl_global_forward / _backward_phase / the *_shard entry points with the helpers of tests/direct_ref.py, at the
shapes of tests/dgl_reduction_cases.py (held to the rule's conditioning by tests/test_dgl_reductions_host.py).

1. exact sums: integer series, weights and bias make every conv1 output an integer of at most 22, so BatchNorm1's sum and sum of squares
   are exact in float32 in ANY order and a dropped, duplicated or mis-routed lane moves the stored mean / rstd by far more than the one
   float32 ulp allowed; the stored bf16 rows must be those integers.  (T - 9 = 1 is not reachable: the entry points need T > 18, so the
   smallest case is T - 9 = 10.)
2. the tolerance rule of tests/test_gpu_dgl_global_direct.py (e_dev <= 8 e_f32 + 3.0e-6; bf16 mode: + 2 e_model) at the new tile edges,
   forward and backward, both modes, and around fc_unpermute's workgroup span with the fc gradient accumulated and stored.  Only
   bf16 mode runs the channels-last kernels; the f32-mode cases run conv_relu_fwd_kernel and its f32 companions at the same shapes.
3. time slices whose bounds are no multiple of a lane's run: the halo (excluded from the statistics) starts inside a run.
4. buffer reuse: the rule of test_buffers_can_be_reused (difference <= 4 x noise + FLOOR).  f32 mode: every tensor, as there.  bf16
   mode (the only one that runs the new kernels): the rule holds for every tensor that does not pass through a STORED bf16 rounding of a
   value that f32 atomics decide -- g, the six running statistics, fc_w, fc_b, bn2_w, bn2_b, bn3_w, bn3_b (these cover conv1 / conv2
   forward and fc_unpermute).  The other six (conv2_w, conv2_b, bn1_w, bn1_b, conv1_w, conv1_b) are sums over dz2, which the mode
   stores rounded to bf16 after BatchNorm2's backward transform, whose two sums per channel come from f32 atomics: where an element of
   dz2 sits next to a rounding boundary the last bit of those sums decides its bf16 value, and the six gradients land in one of two
   or three discrete states.  Measured, eight fresh runs per input, conv1_b to run 0: this build at (13, 4106) seed 0 4.1e-5 in five
   runs and 8e-8 in two, seed 5 1.3e-5 / 8.7e-5 / 5e-8; the PARENT build at (13, 4106) seed 6 4.1e-5 in six runs and 8e-8 in one, at
   (13, 1043) seed 0 2.5e-4 / 4e-8, seed 4 2.5e-5 / 1.1e-6 -- a property of the mode, not of a build or of a buffer.  A single
   fresh pair can sit in one state (noise 1e-7) and the reuse run in the other, so for these six `4 x noise + FLOOR` is not a
   rule; they are held to what bounds a flipped rounding: the operand model (e_dev <= 8 e_f32 + FLOOR + 2 e_model), fresh or reused.
"""
import pytest
import torch

from oracle import step_oracle as O
from tests import direct_ref as D
from tests import dgl_reduction_cases as C

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
M, FLOOR = D.GLOBAL_M, D.GLOBAL_FLOOR
# bf16 mode: sums over the stored bf16 dz2 (see 4. above)
BEHIND_STORED_DZ2 = ("conv2_w", "conv2_b", "bn1_w", "bn1_b", "conv1_w", "conv1_b")


def _refs(N, T):
    return D.cached_global_ref(N, T, F64), D.cached_global_ref(N, T, F32)


def _model(N, T):
    return D.cached_global_model(N, T)


def _held(tag, dev, r64, r32, model=None):
    """every tensor of the device result against float64: e_dev <= M e_f32 + FLOOR, with a model + 2 e_model (the rule of
    tests/test_gpu_dgl_global_direct.py); guard bands intact, everything finite (Compare.add)"""
    fd, f64, f32 = D.flat_global(dev), D.flat_global(r64), D.flat_global(r32)
    assert set(fd) == set(f64), (sorted(fd), sorted(f64))
    fm = None if model is None else D.flat_global(model)
    cmp_ = D.Compare(tag, M, FLOOR, FLOOR)
    for k in fd:
        cmp_.add(k, fd[k], f64[k], f32[k], extra=0.0 if fm is None else 2 * D.rel_l2(fm[k], f64[k]))
    assert dev["guards_intact"], f"{tag}: a guard band behind or in front of saved / work was written"
    cmp_.finish()


# ----------------------------------------------------------------------------------------- 1. exact sums
def _integer_case(N, T):
    c = D.global_case(N, T, seed=7)
    gen = torch.Generator().manual_seed(N * 7919 + T)
    c["series"] = torch.randint(-2, 3, (N, T), generator=gen).float()
    c["p"]["conv1_w"] = torch.randint(-1, 2, (8, 1, 10), generator=gen).float()
    c["p"]["conv1_b"] = torch.randint(-2, 3, (8,), generator=gen).float()
    return c


def _ulps(a, b):
    """distance in float32 steps between two float32 tensors of one sign"""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


@pytest.mark.parametrize("N,T", C.EXACT_SHAPES)
def test_batchnorm1_sums_are_exact_on_integers(N, T):
    c = _integer_case(N, T)
    T1, T2 = T - 9, T - 18
    dev = D.run_global(c, bf16=1, backward=False)
    assert dev["guards_intact"]
    saved = dev["buffers"][0].t
    c1 = torch.relu(torch.nn.functional.conv1d(c["series"].double().unsqueeze(1), c["p"]["conv1_w"].double(), c["p"]["conv1_b"].double()))
    assert float(c1.max()) <= 22 and torch.equal(c1, c1.round())
    a1h = saved[:N * T1 * 4].view(torch.bfloat16).view(N, T1, 8).float().cpu()
    assert torch.equal(a1h, c1.transpose(1, 2).float()), "a1h is not the integer conv1 output"
    st1 = saved[N * 8 * T1 + N * 16 * T2 + N * 100:][:32].cpu()
    mean = c1.mean((0, 2))
    var = (c1 * c1).mean((0, 2)) - mean * mean
    rstd = (var.clamp_min(0) + O.BN_EPS).rsqrt()
    u_mean, u_rstd = _ulps(st1[16:24], mean.float()), _ulps(st1[24:32], rstd.float())
    print(f"EXACT N={N} T={T} mean ulps {u_mean.tolist()} rstd ulps {u_rstd.tolist()}")
    assert int(u_mean.max()) <= 1 and int(u_rstd.max()) <= 1, (st1[16:32], mean, rstd)


# ----------------------------------------------------------------------------------------- 2. the tolerance rule at the new edges
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("N,T", C.EDGE_SHAPES)
def test_conv1_tile_edges_within_the_rule(N, T, bf16):
    dev = D.run_global(D.cached_global_case(N, T), bf16=bf16)
    _held(f"edges bf16={bf16} N={N} T={T}", dev, *_refs(N, T), model=_model(N, T) if bf16 else None)


@pytest.mark.parametrize("fresh_fc", [False, True])
@pytest.mark.parametrize("N,T", C.FC_SHAPES)
def test_fc_unpermute_span_edges_within_the_rule(N, T, fresh_fc):
    """fresh_fc: grads.fc_w starts as NaN bytes and is stored (overwrite); otherwise it accumulates into zeros"""
    dev = D.run_global(D.cached_global_case(N, T), bf16=1, fresh_fc=fresh_fc)
    _held(f"fc span fresh_fc={fresh_fc} N={N} T={T}", dev, *_refs(N, T), model=_model(N, T))


# ----------------------------------------------------------------------------------------- 3. time slices
@pytest.mark.parametrize("N,T,bounds", C.SLICED)
def test_time_slices_with_a_halo_inside_a_run(N, T, bounds):
    assert all(b % C.RUN for _, b in bounds[:-1])
    dev = D.run_global_sliced(D.cached_global_case(N, T), bounds)
    _held(f"sliced N={N} T={T} {bounds}", dev, *_refs(N, T), model=_model(N, T))


# ----------------------------------------------------------------------------------------- 4. buffer reuse
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("N,T", C.REUSE_SHAPES)
def test_buffers_can_be_reused_at_a_tile_edge(N, T, bf16):
    c = D.cached_global_case(N, T)
    a, b = D.run_global(c, bf16=bf16), D.run_global(c, bf16=bf16)
    again = D.run_global(c, bf16=bf16, buffers=D.run_global(c, bf16=bf16)["buffers"])
    _held(f"reuse bf16={bf16} N={N} T={T}", again, *_refs(N, T), model=_model(N, T) if bf16 else None)
    fa, fb, fx = D.flat_global(a), D.flat_global(b), D.flat_global(again)
    bad = []
    for k in fa:
        noise, reuse = D.rel_l2(fb[k], fa[k]), D.rel_l2(fx[k], fa[k])
        if noise > 0 or reuse > 0:
            print(f"NOISE bf16={bf16} N={N} T={T} {k:<8s} fresh-vs-fresh {noise:.3e} reuse-vs-fresh {reuse:.3e}")
        if bf16 and k in BEHIND_STORED_DZ2:
            continue          # two or three discrete states per input in this mode (docstring, 4.): held to the model above
        if not reuse <= 4 * noise + FLOOR:
            bad.append((k, noise, reuse))
    assert not bad, bad
