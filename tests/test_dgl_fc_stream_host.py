"""Conditioning of the shapes of tests/test_gpu_dgl_fc_stream.py, checked on the host the way tests/test_direct_ref_host.py checks
direct_ref.GLOBAL_SHAPES: the tolerance rule of the direct tests only means something on well-conditioned inputs."""
import pytest
import torch

from tests import direct_ref as D
from tests import dgl_fc_stream_shapes as S


@pytest.mark.parametrize("N,T", S.ALL_SHAPES)
def test_fc_stream_cases_are_well_conditioned(N, T):
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


def test_shape_helpers_put_the_cases_on_the_edges():
    """the ranges and workgroups the comments of dgl_fc_stream_shapes.py promise"""
    assert S.fwd_ranges(13, 80) == (20, 4, 5) and S.fwd_ranges(13, 81) == (21, 5, 5) and S.fwd_ranges(13, 79) == (20, 4, 5)
    assert S.fwd_ranges(13, 770) == (193, 5, 39)
    assert S.fwd_ranges(13, 3)[2] == 1 and S.fwd_ranges(13, 5) == (2, 2, 1)
    assert S.wgrad_groups(511) == (256, 1, 256) and S.wgrad_groups(512) == (256, 1, 256) and S.wgrad_groups(513) == (257, 2, 129)
    assert S.wgrad_groups(1) == (1, 1, 1) and S.wgrad_groups(3) == (2, 1, 2)
