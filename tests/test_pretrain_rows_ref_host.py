"""Host checks of tests/pretrain_rows_ref.py, the references of tests/test_gpu_pretrain_rows_direct.py (no GPU):

1. the keep model draws at the rate 1 - p, and its stream depends on the site and on BOTH seed words;
2. the tolerance rule is conditioned: at every case the bound M * e_f32 + FLOOR a tensor is held to is at or below 1e-4 (the cap
   tests/test_direct_ref_host.py sets) and at or below the fixed bound tests/test_gpu_pretrain.py already asserts for that tensor
   (2e-6 for y / stats / dx, 2e-5 for the column sums, 1e-5 for the embedding and decoder-input gradients);
3. the rule has teeth: float64 "wrong kernels" (pretrain_rows_ref.ln_wrong, ignore_site, skip_last_slice) are at least ten bounds away.

The ill-conditioned LayerNorm case (a constant row, a row whose mean is 1e3 times its spread) is exempt from 2: its float32 restatement is
itself 1e-5 .. 1e-4 from float64 (that is what the case is for; the rule scales with it)."""
import math

import numpy as np
import pytest
import torch

from tests import pretrain_rows_ref as R

F64, F32 = torch.float64, torch.float32
SEED, S0, S1 = R.SEEDS[1], R.SITES[0], R.SITES[1]


# ----------------------------------------------------------------------------------------- 1. the keep model
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_is_one_minus_p(p):
    n = 96 * 4096
    k = R.keep_mask(n, SEED, S0, p)
    sd = math.sqrt(p * (1 - p) / n)
    assert abs(float(k.mean()) - (1 - p)) <= 4 * sd, (float(k.mean()), sd)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_stream_depends_on_site_and_on_the_high_seed_word(p):
    n = 96 * 4096
    a, b, c = R.keep_mask(n, SEED, S0, p), R.keep_mask(n, SEED, S0 + 1, p), R.keep_mask(n, SEED ^ (1 << 32), S0, p)
    q = 2 * p * (1 - p)
    sd = math.sqrt(q * (1 - q) / n)
    for name, (u, v) in {"site": (a, b), "seed high word": (a, c), "both": (b, c)}.items():
        share = float((u != v).mean())
        assert abs(share - q) <= 4 * sd, (name, share, q, sd)


def test_keep_model_is_elementwise_and_p_zero_keeps_everything():
    whole = R.keep_mask(1027, SEED, S0, 0.5)
    assert np.array_equal(whole[5:1000], R.keep_mask(995, SEED, S0, 0.5, first=5))          # element i, wherever the call starts
    assert R.keep_mask(1027, SEED, S0, 0.0).all()
    assert R.keep_mult(0.0) == 1.0 and R.keep_mult(0.5) == 2.0 and R.keep_mult(0.1) == float(np.float32(1) / np.float32(0.9))
    assert R.SEEDS[0] & 0xFFFFFFFF == R.SEEDS[1] & 0xFFFFFFFF and R.SEEDS[0] != R.SEEDS[1] and 0 not in R.SITES


def test_layer_norm_restatement_is_torch_layer_norm():
    c = R.cached_ln_case(9)
    want = torch.nn.functional.layer_norm(c["a"].double(), (R.D,), c["gamma"].double(), c["beta"].double(), R.LN_EPS)
    assert R.rel_l2(R.layer_norm(c["a"].double(), c["gamma"].double(), c["beta"].double())[0], want) < 1e-14


# ----------------------------------------------------------------------------------------- 2. conditioning
def _conditions(errs, fixed):
    for name, e in errs.items():
        b = R.bound(fixed.get("kind", True) if name in fixed["sums"] else False, e)
        cap = min(R.FIXED_ANY, fixed["sums"].get(name, fixed["rows"].get(name, R.FIXED_ANY)))
        assert b <= cap, (name, e, b, cap)


def _ln_refs(Rows, p):
    """Rows: a row count, or the tuple of the pooled ones"""
    if isinstance(Rows, tuple):
        return R.pooled([R.cached_ln_ref(F64, r, p) for r in Rows]), R.pooled([R.cached_ln_ref(F32, r, p) for r in Rows])
    return R.cached_ln_ref(F64, Rows, p), R.cached_ln_ref(F32, Rows, p)


LN_CASES = (R.LN_POOLED,) + R.LN_SINGLE


@pytest.mark.parametrize("p", R.LN_P)
@pytest.mark.parametrize("Rows", LN_CASES)
def test_layernorm_cases_are_well_conditioned(Rows, p):
    r64, r32 = _ln_refs(Rows, p)
    errs = {k: R.rel_l2(r32[k], r64[k]) for k in r64}
    _conditions(errs, {"rows": {k: R.FIXED_ROW for k in R.LN_ROW_TENSORS}, "sums": {k: R.FIXED_SUM for k in R.LN_SUM_TENSORS}, "kind": "ln"})


@pytest.mark.parametrize("p", R.EMBED_P)
@pytest.mark.parametrize("shape", R.EMBED_SHAPES)
def test_embedding_and_decoder_input_cases_are_well_conditioned(shape, p):
    c = R.cached_embed_case(*shape)
    sums = {k: R.FIXED_EMBED for k in ("dw", "db", "dpos", "dmask")}
    for fn, site in ((R.embed_ref, S0), (R.dec_ref, S1)):
        r64, r32 = fn(F64, c, p, SEED, site), fn(F32, c, p, SEED, site)
        _conditions({k: R.rel_l2(r32[k], r64[k]) for k in r64}, {"rows": {"x": R.FIXED_EMBED, "dz": R.FIXED_EMBED}, "sums": sums})


@pytest.mark.parametrize("shape", R.SEQSUM_SHAPES)
def test_sum_over_seq_cases_are_well_conditioned(shape):
    c = R.seqsum_case(*shape, ldp=shape[1] + 2, p_off=1, with_idx=True)
    _conditions({"dvec": R.rel_l2(R.seqsum_ref(F32, c), R.seqsum_ref(F64, c))}, {"rows": {}, "sums": {"dvec": R.FIXED_EMBED}})
    assert R.seq_slices(289, 42)[-1] == (289, 289) and len(R.seq_slices(289, 42)) == 18          # the case with an empty last slice


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_column_sum_cases_are_well_conditioned(rows):
    g = torch.Generator().manual_seed(rows)
    x, g0 = torch.randn(rows, 100, generator=g), torch.randn(100, generator=g)
    _conditions({"out": R.rel_l2(R.colsum_ref(F32, x, g0), R.colsum_ref(F64, x, g0))}, {"rows": {}, "sums": {"out": R.FIXED_SUM}})


def test_ill_conditioned_case_is_what_it_claims():
    c = R.cached_ln_case(R.LN_ILL_ROWS, True)
    r64, r32 = R.cached_ln_ref(F64, R.LN_ILL_ROWS, 0.1, True, True), R.cached_ln_ref(F32, R.LN_ILL_ROWS, 0.1, True, True)
    assert float(c["a"][0].std()) == 0.0 and float((c["a"][8:].mean(1) / c["a"][8:].std(1)).min()) > 700
    assert torch.equal(r64["y"][0], c["beta"].double()) and abs(float(r64["stats"][0, 1]) - R.LN_EPS ** -0.5) < 1e-9
    assert 1e-6 < R.rel_l2(r32["y"], r64["y"]) < 1e-3          # the restatement shares the conditioning: no fixed bound fits this case


# ----------------------------------------------------------------------------------------- 3. the rule has teeth
def _far(name, wrong, r64, r32, is_sum):
    """how many bounds the wrong result is away; a result with a zero bound (the float32 restatement is exact) counts by its error alone"""
    b = R.bound(is_sum, R.rel_l2(r32, r64))
    e = R.rel_l2(wrong, r64)
    print(f"WRONG {name}: error {e:.3e}, bound {b:.3e}")
    return e / b if b > 0 else (float("inf") if e > 0 else 0.0)


@pytest.mark.parametrize("Rows", LN_CASES)
def test_wrong_layernorms_are_ten_bounds_away(Rows):
    p = 0.1
    r64, r32 = _ln_refs(Rows, p)
    broken = {"no_xhat_term": ("dx", "dx_dropped"), "eps": ("y", "stats", "dx"), "unbiased": ("y", "stats", "dx"),
              "site": ("pre", "dx_dropped")}
    if not isinstance(Rows, tuple) and Rows > R.LN_CAP_ROWS:          # (a second pass exists)
        broken["stride_tail"] = ("dx", "dx_dropped", "dgamma", "dbeta", "out_colsum")
    for kind, names in broken.items():
        if isinstance(Rows, tuple):
            w = R.pooled([R.ln_wrong(kind, R.cached_ln_case(r), p, SEED, S0, S1) for r in Rows])
        else:
            w = R.ln_wrong(kind, R.cached_ln_case(Rows), p, SEED, S0, S1)
        near = {k: d for k in names if (d := _far(f"{kind} {k} R={Rows}", w[k], r64[k], r32[k], "ln" if k in R.LN_SUM_TENSORS else False)) < 10}
        assert not near, (kind, Rows, near)


@pytest.mark.parametrize("n", R.DROP_N)
def test_a_keep_model_that_ignores_the_site_is_caught(n):
    c = R.drop_case(n)
    differs = 0
    for p in (0.1, 0.5):
        right, wrong = R.keep_mask(n, SEED, S0, p), R.keep_mask(n, SEED, 0, p)
        differs += int((right != wrong).sum())
        if n >= 1023:          # (the exact comparison of the kept set catches ONE differing element; the values say the same, by far)
            r64, r32, w = R.drop_ref(F64, c, p, SEED, S0), R.drop_ref(F32, c, p, SEED, S0), R.drop_ref(F64, c, p, SEED, S0, ignore_site=True)
            for k in ("dropout", "add_dropout", "dropout_relu"):
                assert _far(f"site {k} n={n} p={p}", w[k], r64[k], r32[k], False) >= 10, k
    assert differs > 0 or n < 1023


@pytest.mark.parametrize("p", [0.5])
@pytest.mark.parametrize("shape", R.EMBED_SHAPES)
def test_embedding_with_a_site_blind_stream_is_caught(shape, p):
    c = R.cached_embed_case(*shape)
    for fn, site, names, sums in ((R.embed_ref, S0, ("x", "dw", "db", "dpos"), ("dw", "db", "dpos")),
                                  (R.dec_ref, S1, ("out", "dm", "dpos", "dmask"), ("dpos", "dmask"))):
        r64, r32, w = fn(F64, c, p, SEED, site), fn(F32, c, p, SEED, site), fn(F64, c, p, SEED, site, ignore_site=True)
        for k in names:
            assert _far(f"site {k} {shape}", w[k], r64[k], r32[k], k in sums) >= 10, k


@pytest.mark.parametrize("shape", [s for s in R.SEQSUM_SHAPES if s != (289, 42)])          # (there the last slice is empty: nothing to skip)
def test_a_sum_over_seq_that_skips_its_last_slice_is_caught(shape):
    c = R.seqsum_case(*shape, ldp=shape[1], p_off=0, with_idx=False)
    touched = slice(0, shape[1])
    assert _far(f"last slice {shape}", R.seqsum_ref(F64, c, skip_last_slice=True)[touched], R.seqsum_ref(F64, c)[touched],
                R.seqsum_ref(F32, c)[touched], True) >= 10
