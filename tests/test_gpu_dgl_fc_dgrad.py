"""The graph learner's fc input gradient with BatchNorm2's backward and conv2's ReLU mask on the streaming kernel
(step_amd/csrc/dgl_fc_stream.hip, fc_stream_dgrad_kernel), directly through ``step_dgl_fc_dgrad`` on chosen inputs and through the
library's forward + backward (tests/direct_ref.py), bf16 mode.

Direct (test_direct_*): for n < N, k < K, c = k mod 16

    v = sum_o bf16(dgpre[n][o]) wp[o][k],  x = a2h[n][k],  dz2h[n][k] = bf16( x > 0 ? v - km1 - (x - mu) km2 : 0 )

against the same formula in float64 from the same rounded operands, with km1 / km2 / mu formed in f32.  Exact: bitwise +0 wherever
x <= 0 (+0, -0 and negative values are in the input), the NaN guard bands around dz2h intact, every element with x > 0 finite.  Values:
per element |dev - ref| <= 2^-8 |ref| + M 2^-24 (sum_o |a w| + |km1| + |(x - mu) km2|): one bf16 rounding, plus f32 accumulation and
epilogue.  M is not guessed: the staged GEMM (STEP_DGL_FC_STREAM=0) runs through the same entry on the same inputs and the smallest M it
needs, worst over DIRECT_SHAPES, is M_STAGED; the streaming kernel is allowed twice that, since only the summation order may differ.
MEASURED (MI355X): staged 0.247, streaming 0.247; the bound is M_STREAM = 0.494 (below).

The two paths on identical inputs: the kernel keeps the staged GEMM's products (the same instruction, dgpre as its first operand, o
ascending in 16-wide products) and its epilogue expression, and test_direct_paths_bit_identical asserts that the stored bits are equal.

Shapes (tests/dgl_fc_dgrad_shapes.py): T - 18 around one column tile and a full ring, 256 tiles on 256 workgroups, 257 tiles (pairs, the
last workgroup one ragged tile), three row tiles with 85 and 86 tiles, workgroups of five and four tiles (the ring turns), 960 and 961
nodes (the dispatch rule's two sides); N = 1, 13, 319, 320, 321, 641, 307.

Through the library (test_library_*): every tensor of a forward + backward against float64 under the bf16 rule of
tests/test_gpu_dgl_global_direct.py (GLOBAL_M, GLOBAL_FLOOR), with two-phase backward, accumulation into filled gradients, buffer reuse
and two time slices; and conv1_* / conv2_* / bn1_* -- everything behind dz2h -- agree between the two settings of the switch within
4 x max(the staged path's fresh-vs-fresh spread, e_f32).

Dispatch: graphs of more than three row tiles (N > 960) keep the staged GEMM (dgl_fc_stream_dgrad_ok, profiles/dgl_fc_dgrad_after.md).
The paths store the same bits, so results cannot tell them apart: tests/test_dgl_fc_dgrad_host.py pins both sides through
step_dgl_fc_dgrad_streams, and test_dispatch_rule_on_the_device runs both sides.
"""
import ctypes

import pytest
import torch

from tests import direct_ref as D
from tests import dgl_fc_dgrad_shapes as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EMB = 100
GUARD = 4096                       # bf16 elements of NaN on either side of dz2h (a multiple of 8: dz2h stays 16-byte aligned)
# MEASURED (MI355X), smallest M per path, worst over DIRECT_SHAPES (641 nodes, T - 18 = 1100; 0 at every shape of fewer than 50 000
# open elements): staged GEMM 0.247, streaming kernel 0.247 (equal: the stored bits are).  The streaming kernel's bound is twice the
# staged path's M.
M_STAGED_MEASURED, M_STREAM_MEASURED = 0.247, 0.247
M_STREAM = 2 * M_STAGED_MEASURED
BEHIND = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "bn1_w", "bn1_b")


# ----------------------------------------------------------------------------------------- direct
def _inputs(N, T2, seed=0):
    g = torch.Generator().manual_seed(1000 * N + T2 + seed)
    K = 16 * T2
    dgpre = torch.randn(N, EMB, generator=g) * 3e-3
    wp = (torch.randn(EMB, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(N, K, generator=g) * 0.7 + 0.05          # about half <= 0
    u = torch.rand(N, K, generator=g)
    x = torch.where(u < 0.05, torch.zeros(()), x)
    a2h = x.bfloat16()
    a2h.view(torch.int16)[(u >= 0.05) & (u < 0.10)] = -32768      # -0
    coef = torch.cat([torch.randn(16, generator=g) * 2e-3, torch.randn(16, generator=g) * 2e-3, 0.5 + torch.rand(16, generator=g),
                      torch.zeros(16)])
    st2 = torch.cat([torch.zeros(32), torch.rand(16, generator=g) * 0.5, 0.5 + 2.0 * torch.rand(16, generator=g)])      # mean, rstd > 0
    return dgpre, wp, a2h, coef.float(), st2.float()


_REF = {}


def _reference(N, T2):
    """-> (ref f64 [N][K], S f64 [N][K] the magnitude sum of the bound, x f32) on the device; computed once per shape"""
    if (N, T2) not in _REF:
        dev = torch.device("cuda")
        dgpre, wp, a2h, coef, st2 = (t.to(dev) for t in _inputs(N, T2))
        a = dgpre.bfloat16().double()
        w = wp.double()
        x = a2h.float()
        ch = torch.arange(16 * T2, device=dev) % 16
        km1 = (coef[32 + ch] * coef[ch])
        km2 = (coef[32 + ch] * coef[16 + ch]) * st2[48 + ch]
        mu = st2[32 + ch]
        bn = (x.double() - mu.double()) * km2.double()
        ref = torch.where(x > 0, a @ w - km1.double() - bn, torch.zeros((), dtype=F64, device=dev))
        mag = a.abs() @ w.abs() + km1.double().abs() + bn.abs()
        _REF[(N, T2)] = (ref, mag, x)
    return _REF[(N, T2)]


def _run_direct(N, T2):
    """step_dgl_fc_dgrad on the inputs of the shape -> (bits int16 [N][K], guards intact)"""
    from step_amd import _lib as L
    dev = torch.device("cuda")
    K = 16 * T2
    dgpre, wp, a2h, coef, st2 = (t.to(dev).contiguous() for t in _inputs(N, T2))
    raw = torch.full((N * K + 2 * GUARD,), 0x7FC0, dtype=torch.int16, device=dev)
    out = raw[GUARD:GUARD + N * K]
    assert out.data_ptr() % 16 == 0
    L.call("step_dgl_fc_dgrad", L.ptr(dgpre), L.ptr(wp), L.ptr(a2h), L.ptr(coef), L.ptr(st2), N, K, ctypes.c_void_p(out.data_ptr()), L.stream())
    torch.cuda.synchronize()
    intact = bool((raw[:GUARD] == 0x7FC0).all()) and bool((raw[GUARD + N * K:] == 0x7FC0).all())
    return out.view(N, K).clone(), intact


def _needed_m(bits, N, T2):
    """exact conditions asserted; -> the smallest M of the value condition"""
    ref, mag, x = _reference(N, T2)
    closed = x <= 0
    assert bool((bits[closed] == 0).all()), "an element with x <= 0 is not bitwise +0"
    val = bits.view(torch.bfloat16).double()
    assert bool(torch.isfinite(val[~closed]).all()), "an element with x > 0 is not finite"
    over = ((val - ref).abs() - 2.0 ** -8 * ref.abs()).clamp_min(0.0) / (2.0 ** -24 * mag)
    return float(over[~closed].max()) if bool((~closed).any()) else 0.0


@pytest.mark.parametrize("N,T2", S.DIRECT_SHAPES)
def test_direct_against_float64(N, T2, monkeypatch):
    print(f"SHAPE N={N} T-18={T2}: (tiles, per workgroup, column ranges, row tiles) {S.dgrad_grid(N, T2)}")
    monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
    bits, intact = _run_direct(N, T2)
    assert intact, "a guard band around dz2h was written"
    m_stream = _needed_m(bits, N, T2)
    monkeypatch.setenv("STEP_DGL_FC_STREAM", "0")
    staged, intact0 = _run_direct(N, T2)
    assert intact0
    m_staged = _needed_m(staged, N, T2)
    print(f"NEEDED-M N={N} T-18={T2}: staged {m_staged:.3f} streaming {m_stream:.3f} (bound {M_STREAM})")
    assert m_stream <= M_STREAM, (m_stream, m_staged, M_STREAM)


@pytest.mark.parametrize("N,T2", S.DIRECT_SHAPES)
def test_direct_paths_bit_identical(N, T2, monkeypatch):
    monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
    new, _ = _run_direct(N, T2)
    monkeypatch.setenv("STEP_DGL_FC_STREAM", "0")
    old, _ = _run_direct(N, T2)
    differ = float((new != old).double().mean())
    print(f"PATHS N={N} T-18={T2}: share of elements differing in any bit {differ:.3e}, "
          f"rel_l2 {D.rel_l2(new.view(torch.bfloat16).float(), old.view(torch.bfloat16).float()):.3e}")
    assert torch.equal(new, old)


def test_dispatch_rule_on_the_device(monkeypatch):
    """what the entry point reports it dispatches on, next to a run of each side of the rule"""
    from step_amd import _lib as L
    monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
    edge = S.DG_MAX_RTILES * S.DG_TM
    assert L.lib().step_dgl_fc_dgrad_streams(edge, 80) == 1 and L.lib().step_dgl_fc_dgrad_streams(edge + 1, 80) == 0
    for n in (edge, edge + 1):
        bits, intact = _run_direct(n, 5)
        assert intact and _needed_m(bits, n, 5) <= M_STREAM


# ----------------------------------------------------------------------------------------- through the library
def _refs(N, T):
    return D.cached_global_ref(N, T, F64), D.cached_global_ref(N, T, F32)


def _held(tag, dev, N, T, minus=None):
    """every tensor of the device result against float64 under the bf16 rule; guard bands intact"""
    r64, r32 = _refs(N, T)
    fd, f64, f32, fm = D.flat_global(dev), D.flat_global(r64), D.flat_global(r32), D.flat_global(D.cached_global_model(N, T))
    assert set(fd) == set(f64), (sorted(fd), sorted(f64))
    cmp_ = D.Compare(tag, D.GLOBAL_M, D.GLOBAL_FLOOR, D.GLOBAL_FLOOR)
    for k in fd:
        x = fd[k].double() - minus[k].double() if (minus is not None and k in minus) else fd[k]
        cmp_.add(k, x, f64[k], f32[k], extra=2 * D.rel_l2(fm[k], f64[k]))
    assert dev["guards_intact"], f"{tag}: a guard band behind or in front of saved / work was written"
    cmp_.finish()


def _g0(N, T, seed=5):
    g = torch.Generator().manual_seed(seed)
    r64 = D.cached_global_ref(N, T, F64)
    return {k: (torch.randn(v.shape, generator=g) * max(0.5 * float(v.double().pow(2).mean().sqrt()), 1e-12)).float() for k, v in r64["grads"].items()}


@pytest.mark.parametrize("N,T", S.ALL_LIBRARY_SHAPES)
def test_library_within_the_operand_model_and_paths_agree(N, T, monkeypatch):
    """forward + backward held to float64; what lies behind dz2h agrees between the settings of the switch within
    4 x max(staged fresh-vs-fresh spread, e_f32)"""
    print(f"SHAPE N={N} T-18={T - 18}: {S.dgrad_grid(N, T - 18)}")
    c = D.cached_global_case(N, T)
    r64, r32 = (D.flat_global(r) for r in _refs(N, T))
    monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
    new = D.run_global(c, bf16=1)
    _held(f"fc-dgrad N={N} T={T}", new, N, T)
    monkeypatch.setenv("STEP_DGL_FC_STREAM", "0")
    a, b = D.run_global(c, bf16=1), D.run_global(c, bf16=1)
    assert a["guards_intact"] and b["guards_intact"]
    fn, fa, fb = D.flat_global(new), D.flat_global(a), D.flat_global(b)
    bad = []
    for k in BEHIND:
        spread, e_f32, diff = D.rel_l2(fb[k], fa[k]), D.rel_l2(r32[k], r64[k]), D.rel_l2(fn[k], fa[k])
        base = max(spread, e_f32)
        print(f"AGREE N={N} T={T} {k:<8s} stream-vs-staged {diff:.3e} staged fresh-vs-fresh {spread:.3e} e_f32 {e_f32:.3e} ratio {diff / base:.2f}")
        if not diff <= 4 * base:
            bad.append((k, diff, spread, e_f32))
    assert not bad, bad


def test_library_two_phase_backward():
    N, T = S.SCENARIO
    G0 = _g0(N, T, seed=6)
    dev = D.run_global(D.cached_global_case(N, T), bf16=1, grad_fill=G0, phases=(1, 2))
    for k in BEHIND:
        assert torch.equal(dev["grads_after"][0][k], G0[k]), f"{k} written by phase 1"
    _held(f"phase 1+2 N={N} T={T}", dev, N, T, minus=G0)


def test_library_backward_accumulates_into_the_gradients():
    N, T = S.SCENARIO
    G0 = _g0(N, T)
    dev = D.run_global(D.cached_global_case(N, T), bf16=1, grad_fill=G0)
    for k, v in G0.items():
        assert not torch.equal(dev["grads"][k], v), k
    _held(f"accumulate N={N} T={T}", dev, N, T, minus=G0)


def test_library_buffers_can_be_reused():
    N, T = S.SCENARIO
    c = D.cached_global_case(N, T)
    again = D.run_global(c, bf16=1, buffers=D.run_global(c, bf16=1)["buffers"])
    _held(f"reuse N={N} T={T}", again, N, T)


def test_library_time_slices():
    """two slices of 150 conv2 columns each through the *_shard entry points (backward phase 3 on the kernel, K = 2400 per slice)"""
    N, T = S.SCENARIO
    dev = D.run_global_sliced(D.cached_global_case(N, T), S.SCENARIO_SLICES)
    _held(f"sliced N={N} T={T} {S.SCENARIO_SLICES}", dev, N, T)
