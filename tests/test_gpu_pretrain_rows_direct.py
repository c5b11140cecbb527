"""The pre-training step's row, token and dropout kernels, one by one through the C ABI (step_amd/csrc/pretrain.hip and the tail of
pretrain_fused.hip) on plain tensors -- no TSFormer module -- against tests/pretrain_rows_ref.py in float64, past the grid caps their
strided loops start at: the four LayerNorm kernels (step_pt_layernorm_fwd / _bwd, step_pt_add_layernorm_fwd / step_pt_layernorm_bwd_dropout),
elementwise dropout (step_pt_dropout, step_pt_add_dropout, step_pt_dropout_relu_mask, step_pt_relu_mask), the embedding of the unmasked
tokens and the decoder input (step_pt_embed_unmasked_fwd / _bwd, step_pt_dec_input, step_pt_dec_input_bwd, step_pt_dec_input_bwd_sums),
step_pt_sum_over_seq, step_pt_token_gather / _scatter, step_pt_add_rows, step_colsum, step_pt_colsum_bf16 and step_pt_ffn_wgrad_workgroups.

Conventions of the other direct tests: every output buffer lies between two guard bands and starts as NaN bytes, or as a random G0 where
the contract is `+=`; guards must stay intact, results finite.  Tolerance: the rule of tests/direct_ref.Compare, e_dev = err(device, f64)
<= M * err(f32 restatement, f64) + FLOOR, one RATIO line per tensor and case, printed before anything is asserted.  What is exact carries no
tolerance: the kept set of every dropout site equals the host keep model (pretrain_rows_ref.keep_mask: Philox counter (blk lo, blk hi, site,
0xD20F), key (seed lo, seed hi)) element for element, gather / scatter / add_rows equal the float32 product or sum bit for bit, rows that no
index names keep their G0 bits, the ReLU gate is closed at +0.0, -0.0, negatives and NaN.

MEASURED on an MI355X (two runs of this file; M = 4 x the largest e_dev / e_f32 rounded up to a power of two, FLOOR = the largest difference
between two runs in fresh buffers rounded up to two digits; pretrain_rows_ref.M_ROW / M_SUM / M_SUM_LN / FLOOR_ROW / FLOOR_SUM):
  row-wise   LayerNorm y 1.04-1.05 at R = 4013 .. 24581 (e_dev 3.8e-7 against e_f32 3.6e-7: with rows of mean 3 and spread 0.5 the float32
             row sum of 288 carries the error, on the device as in the restatement), stats 1.04-1.05, dx / dx_dropped 1.00-1.02, pre 1.00; the
             21 rows below one block pooled: y 1.27, stats 1.20, dx 1.10; ill-conditioned case 0.65-1.00 (y: e_dev 3.8e-5 / 4.4e-5).
             Elementwise dropout, embedding x, decoder out / dz / dm: 1.00 (the same single roundings), identical bits in two runs.
             4 x 1.27 -> 8 would break the condition M * e_f32 <= 2e-6 of tests/test_pretrain_rows_ref_host.py at y (8 x 3.65e-7 = 2.9e-6).  No
             kernel is behind the 1.27: it is the draw of 21 rows (0.90 at p = 0, same rows), and every larger case sits at 1.05.  The
             condition is not raised: M_ROW = 4 (3.1 x the largest ratio), FLOOR_ROW = 0.
  LN sums    dbeta of ln_bwd_kernel (2048 blocks of 4 rows, one float32 atomic per block and column, against torch's pairwise sum) 7.02 / 5.70
             at R = 8192, 5.06-5.32 at 8197 / 24581; ln_bwd_drop_kernel (1024 blocks) dbeta 4.81, out_colsum 4.22, dgamma <= 2.8 (both kernels).
             4 x 7.02 -> M_SUM_LN = 32 (largest bound 1.7e-5 <= the 2e-5 of tests/test_gpu_pretrain.py).
  other sums decoder dmask (dec_input_bwd_sums_kernel: 126 x 16 blocks' atomics onto 96 addresses) 5.57 / 6.66 at (300, 168, 42), 2.7 at
             (255, 24, 6); the triple's dmask (step_colsum) 1.8; embedding db 3.39, dw 2.07, dpos <= 1.3; step_pt_sum_over_seq <= 1.00;
             step_colsum 2.57 at 131331 rows, <= 1.5 below; step_pt_colsum_bf16 1.83 (cols = 8), <= 1.12 elsewhere.  4 x 6.66 -> 32 would break
             the 1e-5 of the embedding gradients at dw (e_f32 3.6e-7: 1.26e-5); dmask's e_dev (8.3e-7 .. 1.06e-6) IS its run-to-run spread
             (6.95e-7 / 8.24e-7 between two runs): the order of 2016 atomics, no arithmetic.  Not raised: M_SUM = 16 (2.4 x the largest ratio).
  spread     two runs in fresh buffers: ln_bwd_kernel dgamma 9.05e-7 / 9.77e-7 (the worst of both runs), dbeta 7.9e-7; ln_bwd_drop_kernel
             dgamma 7.3e-7, dbeta 6.6e-7, out_colsum 6.7e-7; dmask 8.2e-7, db 5.0e-7, dw 4.5e-7, dpos 1.2e-7, dvec 9.4e-8, step_colsum 5.3e-7,
             step_pt_colsum_bf16 0 -> FLOOR_SUM = 9.8e-7.  Every row-wise tensor: identical bits.
  exact      kept sets of all dropout sites (96 (n, p, seed, site) combinations x 4 kernels, both LayerNorm sites at 8 + 1 row counts, x / out /
             dm at 6 shapes), gather / scatter / add_rows, untouched rows: no mismatch.
  constant row: max |y - beta| 0 (add_ln_fwd_kernel, with and without b), 3.41e-5 (ln_fwd_kernel: its x - mean is an fma on the unrounded
             288 * float(1 / 96)); bound 1.6e-4 (test_layernorm_kernels_on_a_constant_row_and_a_large_mean).
  mutation   scratch build, ln_bwd_drop_kernel prefetching under row + 2 * stride < R (stale operands in the last pass): R = 8197 and 24581 fail,
             nothing at or below the cap does; keep_scale4 with the site replaced by 0: every kept-set comparison at p > 0 fails."""
import pytest
import torch

from tests import direct_ref as D
from tests import pretrain_rows_ref as R

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DEV = "cuda"
SEED, S0, S1 = R.SEEDS[1], R.SITES[0], R.SITES[1]


def _L():
    from step_amd import _lib
    return _lib


class Out:
    """an output of `shape` between guard bands: NaN bytes, or g0 where the kernel accumulates / works in place"""

    def __init__(self, shape, g0=None):
        self.shape = tuple(shape)
        n = 1
        for d in self.shape:
            n *= d
        self.g = D._Guarded(n, DEV)
        if g0 is not None:
            self.g.t.copy_(g0.reshape(-1).to(F32))

    @property
    def t(self):
        return self.g.t

    def host(self):
        return self.g.t.view(self.shape).cpu()


def _finish(*outs):
    """-> host copies, after the guards of every buffer have been looked at"""
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert o.g.intact(), f"output {i} of shape {o.shape}: a guard band was written"
    return [o.host() for o in outs]


def _dev(t, dtype=F32):
    return t.to(dtype).contiguous().to(DEV)


def _idx(t):
    return None if t is None else t.to(torch.int32).contiguous().to(DEV)


def _cmp(tag, kind=False):
    M, floor = R.rule(kind)
    return D.Compare(tag, M, floor, floor)


class Both:
    """the row-wise and the row-reduced tensors of a case go to their own Compare"""

    def __init__(self, tag, sums, kind=True):
        self.rows, self.sums, self.names = _cmp(tag), _cmp(tag, kind), set(sums)

    def add(self, name, dev, r64, r32, key=None):
        (self.sums if (key or name) in self.names else self.rows).add(name, dev, r64, r32)

    def finish(self):
        self.rows.finish()
        self.sums.finish()


def _same_set(name, got, want, where=None):
    """two boolean tensors are the same set (on `where`), element for element"""
    got, want = torch.as_tensor(got).reshape(-1), torch.as_tensor(want).reshape(-1)
    diff = got != want
    if where is not None:
        diff = diff & torch.as_tensor(where).reshape(-1)
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} of {diff.numel()} keep decisions differ from the host model, first at {int(diff.nonzero()[0])}"


def _keep(shape, seed, site, p):
    n = 1
    for d in shape:
        n *= d
    return torch.from_numpy(R.keep_mask(n, seed, site, p)).view(*shape)


# ----------------------------------------------------------------------------------------- LayerNorm
def run_ln(case, p, seed=SEED, site_fwd=S0, site_bwd=S1, dxd=True, colsum=True):
    """step_pt_add_layernorm_fwd(a, b) -> pre, y, stats, then step_pt_layernorm_bwd_dropout(dy, pre, stats) -> dx, dx_dropped (dxd),
    dgamma / dbeta / out_colsum (colsum) from the case's G0, the way the step chains them"""
    L = _L()
    Rr = case["R"]
    a, b, dy, gamma, beta = (_dev(case[k]) for k in ("a", "b", "dy", "gamma", "beta"))
    pre, y, stats, dx = Out((Rr, 96)), Out((Rr, 96)), Out((Rr, 2)), Out((Rr, 96))
    dxo = Out((Rr, 96)) if dxd else None
    dg, db = Out((96,), case["g0"]["dgamma"]), Out((96,), case["g0"]["dbeta"])
    col = Out((96,), case["g0"]["out_colsum"]) if colsum else None
    st = L.stream()
    L.call("step_pt_add_layernorm_fwd", L.ptr(a), L.ptr(b), Rr, p, seed, site_fwd, L.ptr(gamma), L.ptr(beta), L.ptr(pre.t), L.ptr(y.t), L.ptr(stats.t), st)
    L.call("step_pt_layernorm_bwd_dropout", L.ptr(dy), L.ptr(pre.t), Rr, L.ptr(gamma), L.ptr(stats.t), L.ptr(dx.t), L.ptr(dxo.t) if dxd else None, p, seed,
           site_bwd, L.ptr(dg.t), L.ptr(db.t), L.ptr(col.t) if colsum else None, st)
    outs = [o for o in (pre, y, stats, dx, dxo, dg, db, col) if o is not None]
    names = [n for n, o in zip(("pre", "y", "stats", "dx", "dx_dropped", "dgamma", "dbeta", "out_colsum"), (pre, y, stats, dx, dxo, dg, db, col)) if o is not None]
    return dict(zip(names, _finish(*outs)))


def run_ln_plain(case):
    """LayerNorm of `a` alone: step_pt_add_layernorm_fwd with b = NULL (pre = NULL) -> y_fused, stats_fused; step_pt_layernorm_fwd -> y, stats;
    step_pt_layernorm_bwd(dy, a, stats) -> dx, dgamma, dbeta"""
    L = _L()
    Rr = case["R"]
    a, dy, gamma, beta = (_dev(case[k]) for k in ("a", "dy", "gamma", "beta"))
    y1, s1, y2, s2, dx = Out((Rr, 96)), Out((Rr, 2)), Out((Rr, 96)), Out((Rr, 2)), Out((Rr, 96))
    dg, db = Out((96,), case["g0"]["dgamma"]), Out((96,), case["g0"]["dbeta"])
    st = L.stream()
    L.call("step_pt_add_layernorm_fwd", L.ptr(a), None, Rr, 0.0, 0, 0, L.ptr(gamma), L.ptr(beta), None, L.ptr(y1.t), L.ptr(s1.t), st)
    L.call("step_pt_layernorm_fwd", L.ptr(a), Rr, L.ptr(gamma), L.ptr(beta), L.ptr(y2.t), L.ptr(s2.t), st)
    L.call("step_pt_layernorm_bwd", L.ptr(dy), L.ptr(a), Rr, L.ptr(gamma), L.ptr(s2.t), L.ptr(dx.t), L.ptr(dg.t), L.ptr(db.t), st)
    return dict(zip(("y_fused", "stats_fused", "y", "stats", "dx", "dgamma", "dbeta"), _finish(y1, s1, y2, s2, dx, dg, db)))


def _ln_keep_checks(tag, case, p, dev):
    """the two dropout sites of the fused pair against the host model: b was added where pre != a, dx continued where dx_dropped != 0"""
    Rr = case["R"]
    if "pre" in dev:
        _same_set(f"{tag} pre", dev["pre"] != case["a"], _keep((Rr, 96), SEED, S0, p), where=case["b"].abs() > 1e-3)
    if "dx_dropped" in dev:
        _same_set(f"{tag} dx_dropped", dev["dx_dropped"] != 0, _keep((Rr, 96), SEED, S1, p), where=dev["dx"] != 0)


def _ln_device(Rr, p, ill=False):
    """every LayerNorm call of one case: the fused pair whole, with dx_dropped = NULL, with out_colsum = NULL, and the plain kernels"""
    case = R.cached_ln_case(Rr, ill)
    full = run_ln(case, p)
    _ln_keep_checks(f"R={Rr} p={p}", case, p, full)
    no_dxd, no_col = run_ln(case, p, dxd=False), run_ln(case, p, colsum=False)
    _ln_keep_checks(f"R={Rr} p={p} no colsum", case, p, no_col)
    for k in ("pre", "y", "stats", "dx"):          # the NULL arguments change nothing else (no atomics in these four)
        assert torch.equal(no_dxd[k], full[k]) and torch.equal(no_col[k], full[k]), k
    assert torch.equal(no_col["dx_dropped"], full["dx_dropped"])
    full["out_colsum_plain"] = no_dxd["out_colsum"]
    full["dgamma/no dxd"], full["dbeta/no colsum"] = no_dxd["dgamma"], no_col["dbeta"]
    return full, run_ln_plain(case)


def _ln_compare(tag, dev, plain, r64, r32, p64, p32):
    c = Both(tag, R.LN_SUM_TENSORS, "ln")
    for k in ("pre", "y", "stats", "dx", "dx_dropped", "dgamma", "dbeta", "out_colsum", "out_colsum_plain"):
        c.add(k, dev[k], r64[k], r32[k])
    c.add("dgamma/no dxd", dev["dgamma/no dxd"], r64["dgamma"], r32["dgamma"], key="dgamma")
    c.add("dbeta/no colsum", dev["dbeta/no colsum"], r64["dbeta"], r32["dbeta"], key="dbeta")
    for k, ref in (("y_fused", "y"), ("stats_fused", "stats"), ("y", "y"), ("stats", "stats"), ("dx", "dx"), ("dgamma", "dgamma"), ("dbeta", "dbeta")):
        c.add("plain " + k, plain[k], p64[ref], p32[ref], key=ref)
    c.finish()


@pytest.mark.parametrize("p", R.LN_P)
@pytest.mark.parametrize("Rr", R.LN_SINGLE)
def test_layernorm_kernels_past_their_grid_caps(Rr, p):
    """R = 4013 (the R of tests/test_gpu_pretrain.py), 8192 (exactly the cap of both backward grids), 8197 (a second pass of five rows: the
    prefetch of ln_bwd_drop_kernel taken by five half waves and skipped by the rest), 24581 (three passes, the last ragged)"""
    dev, plain = _ln_device(Rr, p)
    _ln_compare(f"ln R={Rr} p={p}", dev, plain, R.cached_ln_ref(F64, Rr, p), R.cached_ln_ref(F32, Rr, p), R.cached_ln_ref(F64, Rr, 0.0, False),
                R.cached_ln_ref(F32, Rr, 0.0, False))


@pytest.mark.parametrize("p", R.LN_P)
def test_layernorm_kernels_below_one_block(p):
    """R = 1, 3, 8, 9: less than a block, the tails of the 4-row and the 8-row blocks; each run on its own, held to the rule as one tensor
    per name (pretrain_rows_ref.LN_POOLED)"""
    runs = [_ln_device(Rr, p) for Rr in R.LN_POOLED]
    pool = lambda dtype, pp, residual: R.pooled([R.cached_ln_ref(dtype, Rr, pp, residual) for Rr in R.LN_POOLED])
    _ln_compare(f"ln R={R.LN_POOLED} p={p}", R.pooled([d for d, _ in runs]), R.pooled([q for _, q in runs]), pool(F64, p, True), pool(F32, p, True),
                pool(F64, 0.0, False), pool(F32, 0.0, False))


@pytest.mark.parametrize("p", R.LN_P)
def test_layernorm_kernels_on_a_constant_row_and_a_large_mean(p):
    """41 rows, row 0 constant (variance 0: rstd = eps ** -0.5, y = beta), rows 8 .. 40 with a mean 1e3 times their spread; the float32
    restatement has the same conditioning (e_f32 of y: 1e-5 .. 1e-4), so the rule scales itself.  The constant row on its own: a float32 mean
    of 96 threes is within two roundings of 3 (the sum is exact; 1 / 96 and the product round), |x - mean| <= 3 * 2 * 2^-24 = 3.6e-7, times
    rstd = 316.2 and |gamma| <= 1.4: y is within 1.6e-4 of beta.  (ln_fwd_kernel's subtraction is contracted into an fma that sees the
    unrounded product 288 * float(1 / 96) = 3 + 8.9e-8: its y is 2.8e-5 * gamma below beta, measured 3.3e-5; the fused kernel's is beta.)"""
    Rr = R.LN_ILL_ROWS
    dev, plain = _ln_device(Rr, p, ill=True)
    ref = lambda dtype, pp, residual: R.cached_ln_ref(dtype, Rr, pp, residual, True)
    beta = R.cached_ln_case(Rr, True)["beta"]
    for name, y in (("fused", dev["y"]), ("fused, b = NULL", plain["y_fused"]), ("plain", plain["y"])):
        off = float((y[0] - beta).abs().max())
        print(f"constant row, {name}: max |y - beta| = {off:.3e}")
        assert off <= 1.6e-4, (name, off)
    _ln_compare(f"ln ill p={p}", dev, plain, ref(F64, p, True), ref(F32, p, True), ref(F64, 0.0, False), ref(F32, 0.0, False))


# ----------------------------------------------------------------------------------------- elementwise dropout, ReLU masks
def run_dropout(case, p, seed, site):
    L = _L()
    n = case["n"]
    x, a, r = _dev(case["x"]), _dev(case["a"]), _dev(case["relu_of"])
    y, inplace, added, dr, rm = Out((n,)), Out((n,), case["x"]), Out((n,)), Out((n,), case["x"]), Out((n,), case["x"])
    st = L.stream()
    L.call("step_pt_dropout", L.ptr(x), L.ptr(y.t), n, p, seed, site, st)
    L.call("step_pt_dropout", L.ptr(inplace.t), L.ptr(inplace.t), n, p, seed, site, st)
    L.call("step_pt_add_dropout", L.ptr(a), L.ptr(x), L.ptr(added.t), n, p, seed, site, st)
    L.call("step_pt_dropout_relu_mask", L.ptr(dr.t), L.ptr(r), n, p, seed, site, st)
    L.call("step_pt_relu_mask", L.ptr(rm.t), L.ptr(r), n, st)
    return dict(zip(("dropout", "in_place", "add_dropout", "dropout_relu", "relu"), _finish(y, inplace, added, dr, rm)))


@pytest.mark.parametrize("n", R.DROP_N)
def test_elementwise_dropout_and_relu_masks(n):
    """n on the scalar tail (1, 3, 5, 1023, 1027) and on the 1024-element block edge; p = 0, 0.1, 0.5; two seeds that differ in the high word
    only, two sites: the kept set IS the host model's, element for element"""
    case = R.drop_case(n)
    assert bool((case["x"] != 0).all())
    gate = R.open_gate(case["relu_of"])
    assert not bool(gate[torch.isnan(case["relu_of"]) | (case["relu_of"] == 0)].any())          # NaN, +0.0 and -0.0 are closed
    for p in R.DROP_P:
        for seed in R.SEEDS:
            for site in R.SITES:
                tag = f"drop n={n} p={p} seed={seed >> 32} site={site}"
                dev = run_dropout(case, p, seed, site)
                keep = _keep((n,), seed, site, p)
                _same_set(tag + " dropout", dev["dropout"] != 0, keep)
                _same_set(tag + " add_dropout", dev["add_dropout"] != case["a"], keep, where=case["x"].abs() > 1e-4)
                _same_set(tag + " dropout_relu", dev["dropout_relu"] != 0, keep & gate)
                _same_set(tag + " relu", dev["relu"] != 0, gate)
                assert torch.equal(dev["in_place"], dev["dropout"])
                r64, r32 = R.drop_ref(F64, case, p, seed, site), R.drop_ref(F32, case, p, seed, site)
                c = _cmp(tag)
                for k in ("dropout", "add_dropout", "dropout_relu", "relu"):
                    c.add(k, dev[k], r64[k], r32[k])
                c.finish()


# ----------------------------------------------------------------------------------------- embedding, decoder input
EMBED_SUMS = ("dpos", "dw", "db", "dmask")


def run_embed(c, p, seed=SEED, site=S0):
    L = _L()
    S, P, Pu = c["S"], c["P"], c["Pu"]
    series, w, b, pos, dxg, um = _dev(c["series"]), _dev(c["w"]), _dev(c["b"]), _dev(c["pos"]), _dev(c["dx"]), _idx(c["um"])
    x = Out((S, Pu, 96))
    dpos, dw, db = Out(c["pos"].shape, c["g0"]["dpos"]), Out((96, 12), c["g0"]["dw"]), Out((96,), c["g0"]["db"])
    st = L.stream()
    L.call("step_pt_embed_unmasked_fwd", L.ptr(series), L.ptr(um), L.ptr(w), L.ptr(b), L.ptr(pos), S, 12 * P, Pu, p, seed, site, L.ptr(x.t), st)
    L.call("step_pt_embed_unmasked_bwd", L.ptr(dxg), L.ptr(series), L.ptr(um), S, 12 * P, Pu, p, seed, site, L.ptr(dpos.t), L.ptr(dw.t), L.ptr(db.t), st)
    return dict(zip(("x", "dpos", "dw", "db"), _finish(x, dpos, dw, db)))


def run_dec(c, p, seed=SEED, site=S1):
    """step_pt_dec_input -> out; step_pt_dec_input_bwd_sums -> dz, dpos, dmask; and the layer-by-layer path's triple step_pt_dec_input_bwd ->
    dz, dm, step_pt_sum_over_seq(dm, mk) -> dpos, step_colsum(dm) -> dmask"""
    L = _L()
    S, P, Pu = c["S"], c["P"], c["Pu"]
    Pm = P - Pu
    z, mt, pos, dout, mk = _dev(c["z"]), _dev(c["mask_token"]), _dev(c["pos"]), _dev(c["dout"]), _idx(c["mk"])
    out, dz, dz3, dm = Out((S, P, 96)), Out((S, Pu, 96)), Out((S, Pu, 96)), Out((S, Pm, 96))
    dpos, dmask = Out(c["pos"].shape, c["g0"]["dpos"]), Out((96,), c["g0"]["dmask"])
    dpos3, dmask3 = Out(c["pos"].shape, c["g0"]["dpos"]), Out((96,), c["g0"]["dmask"])
    st = L.stream()
    L.call("step_pt_dec_input", L.ptr(z), L.ptr(mt), L.ptr(pos), L.ptr(mk), S, P, Pu, p, seed, site, L.ptr(out.t), st)
    L.call("step_pt_dec_input_bwd_sums", L.ptr(dout), S, P, Pu, p, seed, site, L.ptr(mk), L.ptr(dz.t), L.ptr(dpos.t), L.ptr(dmask.t), st)
    L.call("step_pt_dec_input_bwd", L.ptr(dout), S, P, Pu, p, seed, site, L.ptr(dz3.t), L.ptr(dm.t), st)
    L.call("step_pt_sum_over_seq", L.ptr(dm.t), S, Pm, 0, Pm, L.ptr(mk), L.ptr(dpos3.t), st)
    L.call("step_colsum", L.ptr(dm.t), S * Pm, 96, 96, L.ptr(dmask3.t), st)
    return dict(zip(("out", "dz", "dz/triple", "dm", "dpos", "dmask", "dpos/triple", "dmask/triple"), _finish(out, dz, dz3, dm, dpos, dmask, dpos3, dmask3)))


def _untouched(name, dev, g0, rows):
    """rows of an accumulated table that no index names keep the bits they had"""
    rest = torch.ones(g0.shape[0], dtype=torch.bool)
    rest[rows] = False
    assert int(rest.sum()) >= R.NPOS_EXTRA
    assert torch.equal(dev[rest].view(torch.int32), g0[rest].view(torch.int32)), f"{name}: a row outside the index list changed"


@pytest.mark.parametrize("p", R.EMBED_P)
@pytest.mark.parametrize("shape", R.EMBED_SHAPES)
def test_embedding_and_decoder_input(shape, p):
    """(S, P, Pu): S = 1; 37 (tests/test_gpu_pretrain.py: three blocks in y, one sequence per thread); 255 / 256 / 517 (gridDim.y = 16 and the
    strided sequence loop of the two backward kernels); config C3's 168 tokens.  Keep decisions from the host model."""
    c = R.cached_embed_case(*shape)
    S, P, Pu = shape
    tag = f"S={S} P={P} Pu={Pu} p={p}"
    dev = run_embed(c, p)
    r64, r32 = R.embed_ref(F64, c, p, SEED, S0), R.embed_ref(F32, c, p, SEED, S0)
    _same_set(tag + " x", dev["x"] != 0, _keep((S, Pu, 96), SEED, S0, p), where=r64["x"].abs() > 0 if p == 0 else None)
    _untouched(tag + " embedding dpos", dev["dpos"], c["g0"]["dpos"], c["um"])
    cmp = Both("embed " + tag, EMBED_SUMS)
    cmp.add("x", dev["x"], r64["x"], r32["x"])
    cmp.add("dpos", dev["dpos"][c["um"]], r64["dpos"][c["um"]], r32["dpos"][c["um"]])
    cmp.add("dw", dev["dw"], r64["dw"], r32["dw"])
    cmp.add("db", dev["db"], r64["db"], r32["db"])
    cmp.finish()

    dev = run_dec(c, p)
    r64, r32 = R.dec_ref(F64, c, p, SEED, S1), R.dec_ref(F32, c, p, SEED, S1)
    keep = _keep((S, P, 96), SEED, S1, p)[:, Pu:]
    _same_set(tag + " out", dev["out"][:, Pu:] != 0, keep)
    _same_set(tag + " dm", dev["dm"] != 0, keep)
    assert torch.equal(dev["dz/triple"], dev["dz"])
    cmp = Both("dec " + tag, EMBED_SUMS + ("dpos/triple", "dmask/triple"))
    for k in ("out", "dz", "dm", "dmask"):
        cmp.add(k, dev[k], r64[k], r32[k])
    cmp.add("dmask/triple", dev["dmask/triple"], r64["dmask"], r32["dmask"])
    for k in ("dpos", "dpos/triple"):
        _untouched(f"{tag} decoder {k}", dev[k], c["g0"]["dpos"], c["mk"])
        cmp.add(k, dev[k][c["mk"]], r64["dpos"][c["mk"]], r32["dpos"][c["mk"]])
    cmp.finish()


# ----------------------------------------------------------------------------------------- step_pt_sum_over_seq
def run_seqsum(c):
    L = _L()
    dvec, dx, idx = Out(c["g0"].shape, c["g0"]), _dev(c["dx"]), _idx(c["idx"])
    L.call("step_pt_sum_over_seq", L.ptr(dx), c["S"], c["ldp"], c["p_off"], c["p_cnt"], L.ptr(idx), L.ptr(dvec.t), L.stream())
    return _finish(dvec)[0]


@pytest.mark.parametrize("shape", R.SEQSUM_SHAPES)
def test_sum_over_seq(shape):
    """(S, p_cnt): one slice (1, 15 sequences), three (53), eighteen of 17 with an EMPTY last one (289 x 42), sixteen by the 2048 / p_cnt cap
    (647 x 126); positions at an offset inside wider rows (ldp > p_cnt, p_off > 0), with and without an index list"""
    S, p_cnt = shape
    cmp = _cmp(f"seqsum S={S} p_cnt={p_cnt}", True)
    for ldp, p_off, with_idx in ((p_cnt, 0, False), (p_cnt + 3, 2, True), (p_cnt + 3, 3, False), (p_cnt, 0, True)):
        c = R.seqsum_case(S, p_cnt, ldp, p_off, with_idx)
        dev = run_seqsum(c)
        rows = c["idx"] if with_idx else torch.arange(p_cnt)
        _untouched(f"seqsum {shape} ldp={ldp} p_off={p_off} idx={with_idx}", dev, c["g0"], rows)
        cmp.add(f"dvec ldp={ldp} off={p_off} idx={int(with_idx)}", dev[rows], R.seqsum_ref(F64, c)[rows], R.seqsum_ref(F32, c)[rows])
    cmp.finish()


# ----------------------------------------------------------------------------------------- gather, scatter, add_rows
SENTINEL = 12345.0


@pytest.mark.parametrize("shape", R.TOKEN_SHAPES)
def test_token_gather_scatter_and_add_rows_are_exact(shape):
    L = _L()
    S, P, T = shape
    g = torch.Generator().manual_seed(S * 1000 + P)
    src, ddst, vec = torch.randn(S, P, 96, generator=g), torch.randn(S, T, 96, generator=g), torch.randn(P + 5, 96, generator=g)
    idx, ridx = torch.randperm(P, generator=g)[:T].contiguous(), torch.randperm(P + 5, generator=g)[:P].contiguous()
    st = L.stream()
    d_src, d_ddst, d_idx = _dev(src), _dev(ddst), _idx(idx)
    for scale in (float(torch.tensor(96.0).sqrt()), 1.0):
        dst, dsrc = Out((S, T, 96)), Out((S, P, 96), torch.full((S, P, 96), SENTINEL))
        L.call("step_pt_token_gather", L.ptr(d_src), S, P, L.ptr(d_idx), T, scale, L.ptr(dst.t), st)
        L.call("step_pt_token_scatter", L.ptr(d_ddst), S, P, L.ptr(d_idx), T, scale, L.ptr(dsrc.t), st)
        got_dst, got_dsrc = _finish(dst, dsrc)
        s32 = torch.tensor(scale, dtype=F32)
        assert torch.equal(got_dst, src[:, idx] * s32), f"gather {shape} scale={scale}"          # one float32 product: no other rounding to take
        want = torch.full((S, P, 96), SENTINEL)
        want[:, idx] = ddst * s32
        assert torch.equal(got_dsrc, want), f"scatter {shape} scale={scale}"
    for rows, table in ((None, vec[:P].contiguous()), (ridx, vec)):
        x, d_table, d_rows = Out((S, P, 96), src), _dev(table), _idx(rows)
        L.call("step_pt_add_rows", L.ptr(x.t), S, P, L.ptr(d_table), L.ptr(d_rows), st)
        got = _finish(x)[0]
        assert torch.equal(got, src + (table if rows is None else table[rows])), f"add_rows {shape} idx={rows is not None}"


# ----------------------------------------------------------------------------------------- column sums
def _colsum_case(rows, cols, ld):
    g = torch.Generator().manual_seed(rows * 7 + cols + ld)
    x = torch.randn(rows, ld, generator=g)
    x[:, cols:] = float("nan")          # the padding of a row is not the kernel's to read
    return x, torch.randn(cols, generator=g)


def run_colsum(x, g0, cols):
    L = _L()
    out, d_x = Out((cols,), g0), _dev(x)
    L.call("step_colsum", L.ptr(d_x), x.shape[0], cols, x.shape[1], L.ptr(out.t), L.stream())
    return _finish(out)[0]


@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum_f32(rows):
    """rows = 1, 255 (one chunk), 1029 (five), 256 x 513 + 3 (past the cap of 512 chunks: the strided row loop); cols = 1, 96, 100 (two
    column tiles, the second ragged); rows packed (ld = cols) and padded (ld = cols + 28, NaN in the padding)"""
    cmp = _cmp(f"colsum rows={rows}", True)
    dev, r64, r32 = [], [], []
    for cols in R.COLSUM_COLS:
        for ld in (cols, cols + R.COLSUM_PAD):
            x, g0 = _colsum_case(rows, cols, ld)
            dev.append(run_colsum(x, g0, cols))
            r64.append(R.colsum_ref(F64, x[:, :cols], g0))
            r32.append(R.colsum_ref(F32, x[:, :cols], g0))
            print(f"colsum rows={rows} cols={cols} ld={ld}: e_dev={D.rel_l2(dev[-1], r64[-1]):.3e} e_f32={D.rel_l2(r32[-1], r64[-1]):.3e}")
    # one tensor for the rule (cols = 1 is a scalar, whose ONE rounding error can be anything against the restatement's); a wrong scalar
    # is a 394th of it
    cmp.add("out (six calls)", torch.cat(dev), torch.cat(r64), torch.cat(r32))
    cmp.finish()


def run_colsum_bf16(x, g0):
    L = _L()
    out, d_x = Out((x.shape[1],), g0), _dev(x, torch.bfloat16)
    L.call("step_pt_colsum_bf16", L.ptr(d_x), x.shape[0], x.shape[1], L.ptr(out.t), L.stream())
    return _finish(out)[0]


@pytest.mark.parametrize("cols", R.COLSUM16_COLS)
def test_colsum_bf16(cols):
    """cols = 8, 96, 1000, 2048: 256, 21, 2 and 1 row lanes per block (1000: six idle threads); rows = 1, 1023 / 1024 / 1025 (the slab
    edge), 2981 (three slabs, the last ragged).  The operand is bf16: the reference sums the same bf16 values."""
    cmp = _cmp(f"colsum_bf16 cols={cols}", True)
    dev, r64, r32 = [], [], []
    for rows in R.COLSUM16_ROWS:
        g = torch.Generator().manual_seed(rows * 11 + cols)
        x, g0 = torch.randn(rows, cols, generator=g).to(torch.bfloat16), torch.randn(cols, generator=g)
        dev.append(run_colsum_bf16(x, g0))
        r64.append(R.colsum_ref(F64, x, g0))
        r32.append(R.colsum_ref(F32, x, g0))
        print(f"colsum_bf16 cols={cols} rows={rows}: e_dev={D.rel_l2(dev[-1], r64[-1]):.3e} e_f32={D.rel_l2(r32[-1], r64[-1]):.3e}")
    cmp.add("out (five calls)", torch.cat(dev), torch.cat(r64), torch.cat(r32))          # (cols = 8: eight values a call)
    cmp.finish()


# ----------------------------------------------------------------------------------------- workspace of the feed-forward weight gradient
@pytest.mark.parametrize("rows", R.WGRAD_ROWS)
def test_ffn_wgrad_workgroups_size_the_workspace(rows):
    """step_pt_ffn_wgrad_ws_floats(R) is step_pt_ffn_wgrad_workgroups(R) partial results of dW1 [96, 384], dW2 [384, 96] and db1 [384]
    (pretrain_fused.hip states it so); one workgroup per stage of two 32-row tiles, 256 at the most"""
    lib = _L().lib()
    wg = lib.step_pt_ffn_wgrad_workgroups(rows)
    assert wg == min(-(-(-(-rows // 32)) // 2), 256) and wg > 0
    assert lib.step_pt_ffn_wgrad_ws_floats(rows) == wg * (96 * 384 + 384 * 96 + 384)


# ----------------------------------------------------------------------------------------- run-to-run spread (the FLOOR of the sums)
def test_two_runs_in_fresh_buffers():
    """the largest case of every family twice, each time in fresh buffers: row-wise tensors identical bits; the atomically accumulated sums
    differ by the order of their float32 atomics -- the SPREAD lines are where FLOOR_SUM is measured -- and two runs may not be further apart
    than the rule lets ONE run be from float64"""
    spread = {}

    def twice(tag, fn, sums):
        """sums: name -> (float64 reference, float32 restatement)"""
        a, b = fn(), fn()
        for k in a:
            if k in sums:
                r64, r32 = sums[k]
                spread[f"{tag} {k}"] = D.rel_l2(a[k], b[k])
                print(f"SPREAD {tag} {k}: {spread[f'{tag} {k}']:.3e}")
                assert spread[f"{tag} {k}"] <= R.bound("ln" if tag.startswith("ln") else True, D.rel_l2(r32, r64)), (tag, k)
            else:
                assert torch.equal(a[k], b[k]), (tag, k)

    Rr = R.LN_ROWS[-1]
    case = R.cached_ln_case(Rr)
    r64, r32 = R.cached_ln_ref(F64, Rr, 0.1), R.cached_ln_ref(F32, Rr, 0.1)
    twice("ln", lambda: run_ln(case, 0.1), {k: (r64[k], r32[k]) for k in ("dgamma", "dbeta", "out_colsum")})
    r64, r32 = R.cached_ln_ref(F64, Rr, 0.0, False), R.cached_ln_ref(F32, Rr, 0.0, False)
    twice("ln plain", lambda: run_ln_plain(case), {k: (r64[k], r32[k]) for k in ("dgamma", "dbeta")})
    c = R.cached_embed_case(*R.EMBED_SHAPES[-1])
    r64, r32 = R.embed_ref(F64, c, 0.5, SEED, S0), R.embed_ref(F32, c, 0.5, SEED, S0)
    twice("embed", lambda: run_embed(c, 0.5), {k: (r64[k], r32[k]) for k in ("dpos", "dw", "db")})
    r64, r32 = R.dec_ref(F64, c, 0.5, SEED, S1), R.dec_ref(F32, c, 0.5, SEED, S1)
    twice("dec", lambda: run_dec(c, 0.5), {k: (r64[k.split("/")[0]], r32[k.split("/")[0]]) for k in ("dpos", "dmask", "dpos/triple", "dmask/triple")})
    sc = R.seqsum_case(*R.SEQSUM_SHAPES[-1], R.SEQSUM_SHAPES[-1][1], 0, True)
    twice("seqsum", lambda: {"dvec": run_seqsum(sc)}, {"dvec": (R.seqsum_ref(F64, sc), R.seqsum_ref(F32, sc))})
    x, g0 = _colsum_case(R.COLSUM_ROWS[-1], 100, 100)
    twice("colsum", lambda: {"out": run_colsum(x, g0, 100)}, {"out": (R.colsum_ref(F64, x, g0), R.colsum_ref(F32, x, g0))})
    xb = torch.randn(R.COLSUM16_ROWS[-1], 96, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    twice("colsum_bf16", lambda: {"out": run_colsum_bf16(xb, torch.zeros(96))}, {"out": (R.colsum_ref(F64, xb, torch.zeros(96)), R.colsum_ref(F32, xb, torch.zeros(96)))})
    worst = max(spread, key=spread.get)
    print(f"SPREAD worst: {worst} {spread[worst]:.3e}")
