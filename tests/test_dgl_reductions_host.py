"""Conditions on the INPUTS of tests/test_gpu_dgl_reductions.py, as tests/test_direct_ref_host.py holds those of
tests/test_gpu_dgl_global_direct.py: for every shape the tolerance rule is applied to, no BatchNorm channel with a batch variance below
1e-3, and the float32 oracle close enough to float64 that the bound M * e_f32 + FLOOR of every compared tensor stays at or below 1e-4.
No GPU."""
import pytest
import torch

from tests import direct_ref as D
from tests import dgl_reduction_cases as C
from tests.helpers import rel_l2


@pytest.mark.parametrize("N,T", C.TOLERANCE_SHAPES)
def test_reduction_cases_are_well_conditioned(N, T):
    stats = {}
    r64, r32 = D.cached_global_ref(N, T, torch.float64), D.cached_global_ref(N, T, torch.float32)
    D.global_ref(torch.float64, D.cached_global_case(N, T), stats_out=stats)
    count = {"bn1": N * (T - 9), "bn2": N * (T - 18), "bn3": N}
    smallest = min(float((var_u * (count[k] - 1) / count[k]).min()) for k, (_, var_u) in stats.items())
    f64, f32 = D.flat_global(r64), D.flat_global(r32)
    errs = {k: rel_l2(f32[k], f64[k]) for k in f64}
    worst = max(errs, key=errs.get)
    print(f"N={N} T={T}: smallest batch variance {smallest:.2e}, largest e_f32 {errs[worst]:.2e} ({worst})")
    assert smallest >= 1e-3
    assert D.GLOBAL_M * errs[worst] + D.GLOBAL_FLOOR <= 1e-4, (worst, errs[worst])


def test_exact_sum_cases_stay_exact_in_float32():
    """the exact-sums test relies on integer conv1 outputs of at most 22 (ten taps of |series| <= 2 times |weight| <= 1, plus |bias| <= 2:
    it asserts that bound on its own data) whose sum of squares over ONE workgroup's SPAN steps -- one float32 partial row -- stays
    below 2^24 and is therefore exact in any order; across the partial rows bn_finalize_kernel / bn_sums_kernel add in float64"""
    assert 22 * 22 * C.SPAN < 2 ** 24
    assert all(T > 18 for _, T in C.EXACT_SHAPES)
