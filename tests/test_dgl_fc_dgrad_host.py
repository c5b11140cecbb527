"""Host-side checks of tests/test_gpu_dgl_fc_dgrad.py's shapes: the library-path cases are conditioned the way the tolerance rule of the
direct tests needs (as tests/test_dgl_fc_stream_host.py checks its own), and the constants of tests/dgl_fc_dgrad_shapes.py are the
kernel's constexprs and give the grids the comments there promise."""
import os
import re

import pytest
import torch

from tests import direct_ref as D
from tests import dgl_fc_dgrad_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,T", S.ALL_LIBRARY_SHAPES)
def test_fc_dgrad_cases_are_well_conditioned(N, T):
    """no BatchNorm channel with a batch variance below 1e-3, the float32 oracle within 2e-5 relative L2 of float64 on every compared
    tensor, and with them the bound M * e_f32 + FLOOR of every tensor at or below 1e-4"""
    stats = {}
    r64, r32 = D.cached_global_ref(N, T, torch.float64), D.cached_global_ref(N, T, torch.float32)
    D.global_ref(torch.float64, D.cached_global_case(N, T), stats_out=stats)
    count = {"bn1": N * (T - 9), "bn2": N * (T - 18), "bn3": N}
    smallest = min(float((var_u * (count[k] - 1) / count[k]).min()) for k, (_, var_u) in stats.items())
    f64, f32 = D.flat_global(r64), D.flat_global(r32)
    errs = {k: D.rel_l2(f32[k], f64[k]) for k in f64}
    worst = max(errs, key=errs.get)
    print(f"N={N} T={T}: smallest batch variance {smallest:.2e}, largest e_f32 {errs[worst]:.2e} ({worst})")
    assert smallest >= 1e-3
    assert errs[worst] <= 2e-5, (worst, errs[worst])
    assert D.GLOBAL_M * errs[worst] + D.GLOBAL_FLOOR <= 1e-4, (worst, errs[worst])


def _constexpr(src, name):
    m = re.search(r"\b" + name + r"\s*=\s*([A-Z_0-9]+)\b", src)
    assert m, name
    return int(m.group(1)) if m.group(1).isdigit() else _constexpr(src, m.group(1))


def test_shape_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "step_amd", "csrc", "dgl_fc_stream.hip")).read()
    assert tuple(_constexpr(src, n) for n in ("DG_TM", "DG_CT", "DG_RING", "DG_GROUPS", "DG_MAX_RTILES")) == \
        (S.DG_TM, S.DG_CT, S.DG_RING, S.DG_GROUPS, S.DG_MAX_RTILES)


def test_dispatch_rule(monkeypatch):
    """both sides of dgl_fc_stream_dgrad_ok: up to three row tiles on the streaming kernel, four on the staged GEMM; STEP_DGL_FC_STREAM=0
    keeps every size on the staged GEMM.  (The two paths store the same bits, so the rule cannot be pinned on results:
    step_dgl_fc_dgrad_streams reports what step_dgl_fc_dgrad and the backward dispatch on.)"""
    from step_amd import _lib
    lib = _lib.lib()
    monkeypatch.delenv("STEP_DGL_FC_STREAM", raising=False)
    edge = S.DG_MAX_RTILES * S.DG_TM
    assert [lib.step_dgl_fc_dgrad_streams(n, 16 * 300) for n in (1, 307, 883, edge, edge + 1, 4096)] == [1, 1, 1, 1, 0, 0]
    monkeypatch.setenv("STEP_DGL_FC_STREAM", "0")
    assert [lib.step_dgl_fc_dgrad_streams(n, 16 * 300) for n in (307, edge, edge + 1)] == [0, 0, 0]


def test_shape_helpers_put_the_cases_on_the_edges():
    """the grids the comments of dgl_fc_dgrad_shapes.py promise"""
    assert S.dgrad_grid(13, 3) == (1, 1, 1, 1) and S.dgrad_grid(13, 4) == (1, 1, 1, 1) and S.dgrad_grid(13, 5) == (2, 1, 2, 1)
    assert S.dgrad_grid(13, 12) == (3, 1, 3, 1) and S.dgrad_grid(13, 13) == (4, 1, 4, 1)
    assert S.dgrad_grid(13, 1024) == (256, 1, 256, 1) and S.dgrad_grid(13, 1025) == (257, 2, 129, 1)
    assert S.dgrad_grid(641, 340) == (85, 1, 85, 3) and S.dgrad_grid(641, 341) == (86, 2, 43, 3)
    assert S.dgrad_grid(641, 13) == (4, 1, 4, 3) and S.dgrad_grid(13, 4100) == (1025, 5, 205, 1) and S.dgrad_grid(641, 1100) == (275, 4, 69, 3)
    assert {n for n, _ in S.DIRECT_SHAPES} >= {1, 13, 319, 320, 321, 641, 307, 960, 961}
    assert max(n * t2 for n, t2 in S.DIRECT_SHAPES) <= 641 * 1100
