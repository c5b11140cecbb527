"""The streaming kernels of the graph learner's two fc products over a2h (step_amd/csrc/dgl_fc_stream.hip: forward gpre += a2h . wp^T,
weight gradient G = dgpre^T . a2h), reached through ``step_dgl_global_forward`` / ``step_dgl_global_backward_phase`` and the time-sliced
entry points by ctypes (tests/direct_ref.py), bf16 mode.

Shapes (tests/dgl_fc_stream_shapes.py, from the kernels' constexprs FS_TM = 320, FS_KS = 64, FS_RING = 3, WG_TN = 320, WG_CT = 32,
WG_RING = 4): T - 18 one below, at and one above one forward k step, one weight-gradient column tile, a full ring of either kernel, a
forward k range (full, ragged, with ranges that are never launched) and the weight gradient's 256 workgroups; N = 13, 319, 320, 321 and
PEMS04's 307.  tests/test_dgl_fc_stream_host.py holds every shape to the conditioning the rule relies on.  N = 1 cannot be
conditioned -- BatchNorm3's batch variance over one node is exactly 0, g is its bias and every gradient in front of it is 0 -- so one
node only has to run, stay finite, keep the guard bands and agree between the two paths (test_single_node_runs).

Every case is held to the bf16 rule of tests/test_gpu_dgl_global_direct.py, e_dev <= 2 e_model + M e_f32 + FLOOR for every tensor, with
saved and both work buffers exactly step_dgl_global_{saved,work}_floats long between guard bands.

Dispatch rule, pinned on both sides (test_dispatch_rule): the forward kernel takes every shape of the mode; the weight gradient keeps
dgpre^T of ALL nodes resident and takes N <= WG_TN = 320, larger graphs stay on the staged GEMM.  At N = 321 STEP_DGL_FC_STREAM=0
therefore changes g's path but leaves the raw fc weight gradient to the same kernel on both settings.

Agreement of the two paths (STEP_DGL_FC_STREAM=0 against the default) on identical inputs: g, fc_w, bn2_w, bn2_b within 4 x max(the staged
path's own fresh-vs-fresh spread at that shape, e_f32 of that tensor).  Measured worst ratios (difference / that bound's base): see
MEASURED below.
"""
import ctypes

import pytest
import torch

from tests import direct_ref as D
from tests import dgl_fc_stream_shapes as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
M, FLOOR = D.GLOBAL_M, D.GLOBAL_FLOOR
FC_SIDE = ("fc_w", "fc_b", "bn3_w", "bn3_b")
AGREE = ("g", "fc_w", "bn2_w", "bn2_b")
# MEASURED (MI355X), difference between the paths / max(staged fresh-vs-fresh spread, e_f32), worst over AGREEMENT_SHAPES:
#   g 0.11 (13 nodes, T - 18 = 513), fc_w 0.15, bn2_w 0.28 (307 nodes, T - 18 = 300), bn2_b 0.11; bound: 4.  Where both paths cut K into
#   the same ranges (T - 18 = 81 and 300 here) g is bit-identical: the order inside a range is the same, k ascending.


def _refs(N, T):
    return D.cached_global_ref(N, T, F64), D.cached_global_ref(N, T, F32)


def _held(tag, dev, N, T, minus=None, only=None):
    """every tensor of the device result (or those in ``only``) against float64 under the bf16 rule; guard bands intact"""
    r64, r32 = _refs(N, T)
    fd, f64, f32, fm = D.flat_global(dev), D.flat_global(r64), D.flat_global(r32), D.flat_global(D.cached_global_model(N, T))
    assert set(fd) == set(f64), (sorted(fd), sorted(f64))
    cmp_ = D.Compare(tag, M, FLOOR, FLOOR)
    for k in fd:
        if only is not None and k not in only:
            continue
        x = fd[k].double() - minus[k].double() if (minus is not None and k in minus) else fd[k]
        cmp_.add(k, x, f64[k], f32[k], extra=2 * D.rel_l2(fm[k], f64[k]))
    assert dev["guards_intact"], f"{tag}: a guard band behind or in front of saved / work was written"
    cmp_.finish()


def _g0(N, T, seed=5):
    g = torch.Generator().manual_seed(seed)
    r64 = D.cached_global_ref(N, T, F64)
    return {k: (torch.randn(v.shape, generator=g) * max(0.5 * float(v.double().pow(2).mean().sqrt()), 1e-12)).float() for k, v in r64["grads"].items()}


# ----------------------------------------------------------------------------------------- the kernels' edges
@pytest.mark.parametrize("N,T", S.EDGE_SHAPES)
def test_edge_shapes_within_the_operand_model(N, T):
    print(f"SHAPE N={N} T-18={T - 18}: forward (k steps, per range, ranges) {S.fwd_ranges(N, T - 18)}, "
          f"weight gradient (tiles, per workgroup, workgroups) {S.wgrad_groups(T - 18)}")
    _held(f"fc-stream N={N} T={T}", D.run_global(D.cached_global_case(N, T), bf16=1), N, T)


def test_single_node_runs(monkeypatch):
    """N = 1 (see the docstring): finite, guards intact, the same g and fc weight gradient on both paths"""
    c = D.global_case(1, 81 + 18)
    new = D.run_global(c, bf16=1)
    monkeypatch.setenv("STEP_DGL_FC_STREAM", "0")
    old = D.run_global(c, bf16=1)
    for k, v in dict(new["grads"], g=new["g"]).items():          # (BatchNorm3's unbiased running variance over one node is 0 / 0)
        assert bool(torch.isfinite(v).all()), k
    assert new["guards_intact"] and old["guards_intact"]
    assert D.max_abs(new["g"], old["g"]) <= 1e-6 and D.max_abs(new["grads"]["fc_w"], old["grads"]["fc_w"]) <= 1e-6


# ----------------------------------------------------------------------------------------- the two paths on identical inputs
@pytest.mark.parametrize("N,T", S.AGREEMENT_SHAPES)
def test_the_two_paths_agree(N, T, monkeypatch):
    """the paths differ in the order of f32 additions only: per tensor within 4 x max(staged fresh-vs-fresh spread, e_f32)"""
    c = D.cached_global_case(N, T)
    r64, r32 = (D.flat_global(r) for r in _refs(N, T))
    new = D.run_global(c, bf16=1)
    monkeypatch.setenv("STEP_DGL_FC_STREAM", "0")
    a, b = D.run_global(c, bf16=1), D.run_global(c, bf16=1)
    assert new["guards_intact"] and a["guards_intact"] and b["guards_intact"]
    fn, fa, fb = D.flat_global(new), D.flat_global(a), D.flat_global(b)
    bad = []
    for k in AGREE:
        spread, e_f32, diff = D.rel_l2(fb[k], fa[k]), D.rel_l2(r32[k], r64[k]), D.rel_l2(fn[k], fa[k])
        base = max(spread, e_f32)
        print(f"AGREE N={N} T={T} {k:<6s} stream-vs-staged {diff:.3e} staged fresh-vs-fresh {spread:.3e} e_f32 {e_f32:.3e} ratio {diff / base:.2f}")
        if not diff <= 4 * base:
            bad.append((k, diff, spread, e_f32))
    assert not bad, bad


def test_dispatch_rule(monkeypatch):
    """both sides of the weight gradient's rule N <= WG_TN: at 320 nodes the switch changes the raw gradient's summation order (the
    results differ in some bit), at 321 both settings run the staged GEMM on bit-identical operands -- identical up to its own
    run-to-run noise, which is zero for this product (plain stores, no atomics)"""
    out = {}
    for N in (S.WG_TN, S.WG_TN + 1):
        c = D.cached_global_case(N, 81 + 18)
        monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
        fwd = D.run_global(c, bf16=1, backward=False)
        # the backward alone on each setting, from ONE forward's saved buffers: identical dgpre and a2h
        res = []
        for val in (None, "0"):
            if val is None:
                monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
            else:
                monkeypatch.setenv("STEP_DGL_FC_STREAM", val)
            res.append(_backward_only(c, fwd["buffers"]))
        out[N] = torch.equal(res[0], res[1])
        print(f"DISPATCH N={N}: fc_w bit-identical between the settings: {out[N]}, rel_l2 {D.rel_l2(res[0], res[1]):.3e}")
    assert not out[S.WG_TN] and out[S.WG_TN + 1]


def _backward_only(case, buffers):
    """phase 1 of the backward (stored fc weight gradient) in the saved buffer of an earlier forward -> fc_w gradient on the host"""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    dev = torch.device("cuda")
    N, T = case["N"], case["T"]
    lib = L.lib()
    series = case["series"].to(dev).contiguous()
    params = {k: v.to(dev).contiguous().clone() for k, v in case["p"].items()}
    struct = fill_dgl_struct(params, 1)
    dg = case["dg"].to(dev).contiguous()
    grads = {k: torch.zeros_like(params[k]) for k in D.GLOBAL_TRAINABLE}
    gstruct = fill_dgl_struct(grads, 1)
    saved, _, wbwd = buffers
    L.call("step_dgl_global_backward_phase", L.ptr(series), N, T, ctypes.byref(struct), L.ptr(saved.t), L.ptr(dg), L.ptr(wbwd.t),
           ctypes.byref(gstruct), 1 | D.FRESH_FC_GRAD, L.stream())
    torch.cuda.synchronize()
    assert all(b.intact() for b in buffers)
    return grads["fc_w"].cpu()


# ----------------------------------------------------------------------------------------- what callers see, at PEMS04's node count
def test_two_phase_backward():
    N, T = S.SCENARIO
    G0 = _g0(N, T, seed=6)
    dev = D.run_global(D.cached_global_case(N, T), bf16=1, grad_fill=G0, phases=(1, 2))
    first = dict(dev, grads=dev["grads_after"][0])
    for k in D.GLOBAL_TRAINABLE:
        if k not in FC_SIDE:
            assert torch.equal(first["grads"][k], G0[k]), f"{k} written by phase 1"
    _held(f"phase 1 N={N} T={T}", first, N, T, minus=G0, only=FC_SIDE)
    _held(f"phase 1+2 N={N} T={T}", dev, N, T, minus=G0)


@pytest.mark.parametrize("fresh_fc", [False, True])
def test_backward_accumulates_into_the_gradients(fresh_fc):
    N, T = S.SCENARIO
    G0 = _g0(N, T)
    dev = D.run_global(D.cached_global_case(N, T), bf16=1, grad_fill=G0, fresh_fc=fresh_fc)
    for k, v in G0.items():
        assert not torch.equal(dev["grads"][k], v), k
    minus = {k: v for k, v in G0.items() if not (fresh_fc and k == "fc_w")}
    _held(f"accumulate fresh_fc={fresh_fc} N={N} T={T}", dev, N, T, minus=minus)


def test_buffers_can_be_reused():
    """a second forward + backward in the same buffers is held to the reference, and no further from a run in fresh buffers than four
    times the difference of two such runs plus the floor"""
    N, T = S.SCENARIO
    c = D.cached_global_case(N, T)
    a, b = D.run_global(c, bf16=1), D.run_global(c, bf16=1)
    again = D.run_global(c, bf16=1, buffers=D.run_global(c, bf16=1)["buffers"])
    _held(f"reuse N={N} T={T}", again, N, T)
    fa, fb, fx = D.flat_global(a), D.flat_global(b), D.flat_global(again)
    bad = []
    for k in fa:
        noise, reuse = D.rel_l2(fb[k], fa[k]), D.rel_l2(fx[k], fa[k])
        if noise > 0 or reuse > 0:
            print(f"NOISE N={N} T={T} {k:<8s} fresh-vs-fresh {noise:.3e} reuse-vs-fresh {reuse:.3e}")
        if not reuse <= 4 * noise + FLOOR:
            bad.append((k, noise, reuse))
    assert not bad, bad


def test_time_slices():
    """two slices of 150 conv2 columns each through the *_shard entry points (forward phase 3 and backward phase 1 on the kernels)"""
    N, T = S.SCENARIO
    dev = D.run_global_sliced(D.cached_global_case(N, T), S.SCENARIO_SLICES)
    _held(f"sliced N={N} T={T} {S.SCENARIO_SLICES}", dev, N, T)
