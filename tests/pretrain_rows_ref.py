"""Host references of the pre-training step's row, token and dropout kernels (step_amd/csrc/pretrain.hip and the tail of
pretrain_fused.hip): LayerNorm forward / backward with the residual add and the two dropout sites, elementwise dropout and the ReLU masks,
patch + positional embedding of the unmasked tokens, the decoder input, the sums over the sequences and over rows, token gather / scatter.
Imports no GPU.  Shared by tests/test_gpu_pretrain_rows_direct.py (the device side) and tests/test_pretrain_rows_ref_host.py.

Every function takes a ``dtype``: float64 is the reference, float32 the restatement in the precision the kernels claim (the e_f32 of
tests/direct_ref.Compare).  They are written from the model's definitions -- torch.nn.LayerNorm (biased variance, eps = 1e-5) under autograd,
inverted dropout, tsformer.py's patch embedding -> positional embedding -> dropout -> * sqrt(d) -- and not from the kernels: no backward
formula is typed in here, except in the "wrong kernels" at the end, which exist to show that the rule would catch them.

The keep model is the one thing restated from the kernels (it is their contract, include/step_hip.h: "counter-based, replayable"):

    keep(i; seed, site, p):  blk = i >> 2
        r = philox4x32((blk & 0xffffffff, blk >> 32, site, 0xD20F), seed & 0xffffffff, seed >> 32)
        keep  <=>  float32((r[i & 3] >> 8) * 2**-24) >= float32(p);   multiplier float32(1) / (float32(1) - float32(p))

with i the flat element index of the tensor the kernel documents (out [S, P, 96] of the decoder input, x [S, Pu, 96] of the embedding, the
[R, 96] tensor of add-dropout and the LayerNorm kernels) and tests/enc_dropout_host.philox4x32 (known-answer vectors:
tests/test_eval_spread_host.py) as the generator.

M_ROW / M_SUM / FLOOR_ROW / FLOOR_SUM: the tolerance rule's numbers, measured on an MI355X (docstring of tests/test_gpu_pretrain_rows_direct.py).
"""
import functools
import math

import numpy as np
import torch

from tests.enc_dropout_host import philox4x32

D = 96
LN_EPS = 1e-5
SQRT_D = float(np.float32(9.797958971132712))          # the kernels' float constant for sqrt(96)

# ----------------------------------------------------------------------------------------- the tolerance rule's numbers
# row-wise tensors (one thread or one half wave owns an element: y, stats, pre, dx, dx_dropped, x, out, dz, dm, the dropout outputs):
# deterministic, floor 0.  Row-reduced tensors (float32 atomics over blocks, against torch's pairwise float32 sum): the measured run-to-run
# floor and their own M -- M_SUM_LN for the LayerNorm backward's dgamma / dbeta / out_colsum, M_SUM for dpos, dw, db, dmask, dvec and the
# column sums.  Figures and the reasons for M_ROW and M_SUM: docstring of tests/test_gpu_pretrain_rows_direct.py.
M_ROW, FLOOR_ROW = 4.0, 0.0
M_SUM, M_SUM_LN, FLOOR_SUM = 16.0, 32.0, 9.8e-7
# fixed bounds tests/test_gpu_pretrain.py asserts for the same tensors (fused against unfused, or against the forward's own masks); the
# rule's bound must not be looser (tests/test_pretrain_rows_ref_host.py)
FIXED_ROW, FIXED_SUM, FIXED_EMBED, FIXED_ANY = 2e-6, 2e-5, 1e-5, 1e-4

# ----------------------------------------------------------------------------------------- shapes (the smallest that cross each edge)
# LayerNorm rows: less than one block; block tails of the 4-row (ln_fwd / ln_bwd) and the 8-row kernels (add_ln_fwd / ln_bwd_drop); the R of
# tests/test_gpu_pretrain.py; exactly the grid cap of both backward kernels (2048 x 4 = 1024 x 8 = 8192 rows); the first rows of a second
# stride (the prefetch branch taken once, then skipped); three strides with a ragged last one
LN_ROWS = (1, 3, 8, 9, 4013, 8192, 8197, 24581)
LN_CAP_ROWS = 8192
# A tensor of one or a few rows has a handful of rounding errors, and their ratio between two float32 evaluations is luck (e_f32 of y at R = 1:
# 1.3e-6 or 2.0e-7, depending on the draw): the cases below one block are run one by one and held to the rule as ONE tensor per name, their 21
# rows concatenated (tests/test_gpu_optim_direct.py pools its lengths 1 to 5 for the same reason).  A wrong row is a twenty-first of it.
LN_POOLED = tuple(r for r in LN_ROWS if r < 16)
LN_SINGLE = tuple(r for r in LN_ROWS if r >= 16)
LN_P = (0.0, 0.1)
LN_ILL_ROWS = 41         # the ill-conditioned case: row 0 constant, rows 8 .. 40 (from the 8-row kernels' second block on) with a mean 1e3 times their spread
# elementwise dropout: the scalar tail (n % 4 != 0, n < 4) and the 1024-element block edge
DROP_N = (1, 3, 4, 5, 1023, 1024, 1027, 96 * 37)
DROP_P = (0.0, 0.1, 0.5)
SEEDS = (0x0000_0001_2345_6789, 0x0000_0003_2345_6789)          # they differ in the high 32 bits only
SITES = (7, 8)
# embedding / decoder input (S, P, Pu): one sequence; the S of tests/test_gpu_pretrain.py; gridDim.y = 16 with the sequence loop's second
# iteration empty (255: ny = 16 by the other formula), just reached (256), ragged third iteration (517); config C3's token counts
EMBED_SHAPES = ((1, 24, 6), (37, 24, 6), (255, 24, 6), (256, 24, 6), (517, 24, 6), (300, 168, 42))
EMBED_P = (0.0, 0.5)
# step_pt_sum_over_seq (S, p_cnt): one sequence; below 16 (one slice); 3 slices of 18 with a ragged last; 18 slices of 17 whose last is
# EMPTY (17 x 17 = 289); the slice count capped by 2048 / p_cnt (16 slices of 41, ragged last)
SEQSUM_SHAPES = ((1, 5), (15, 5), (53, 5), (289, 42), (647, 126))
TOKEN_SHAPES = ((37, 24, 6), (3, 168, 42))          # (S, P, T) of gather / scatter / add_rows
COLSUM_COLS, COLSUM_PAD, COLSUM_ROWS = (1, 96, 100), 28, (1, 255, 1029, 256 * 513 + 3)          # 512 row chunks of 256 rows is the cap
COLSUM16_COLS, COLSUM16_ROWS = (8, 96, 1000, 2048), (1, 1023, 1024, 1025, 2981)          # 256 / 21 / 2 / 1 row lanes; slabs of 1024 rows
WGRAD_ROWS = (1, 256, 256 * 600 + 45)


def seq_slices(S, p_cnt):
    """the row ranges step_pt_sum_over_seq cuts S sequences into (host code of the entry point): min(2048 // p_cnt, S // 16) slices, at
    least one, of ceil(S / slices) sequences each"""
    n = max(1, min(2048 // p_cnt, S // 16))
    per = -(-S // n)
    return [(min(i * per, S), min((i + 1) * per, S)) for i in range(n)]


def capped_strides(R, rows=LN_CAP_ROWS):
    """[begin, end) of the passes a capped grid of `rows` rows makes over R rows"""
    return [(a, min(a + rows, R)) for a in range(0, R, rows)]


# ----------------------------------------------------------------------------------------- the keep model
def keep_mask(n, seed, site, p, first=0):
    """keep decisions (bool numpy [n]) of elements first .. first + n - 1"""
    blk = np.arange(first >> 2, (first + n + 3) >> 2, dtype=np.uint64)          # one Philox call per four consecutive elements
    c = np.stack([blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), np.full(blk.shape, site, np.uint64), np.full(blk.shape, 0xD20F, np.uint64)], 1)
    r = philox4x32(c.astype(np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    word = r.reshape(-1)[(first & 3):(first & 3) + n]          # element i takes word i & 3 of call i >> 2
    unit = (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return unit >= np.float32(p)


def keep_mult(p):
    """the kept elements' multiplier as the kernels form it, a float32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_tensor(shape, seed, site, p, dtype, ignore_site=False):
    """multiplier tensor (keep ? 1 / (1 - p) : 0) of a tensor of `shape`, elements numbered row-major; p = 0 keeps all.
    ignore_site: the WRONG model whose stream does not depend on the site."""
    n = int(np.prod(shape))
    k = keep_mask(n, seed, 0 if ignore_site else site, p)
    return (torch.from_numpy(k).to(dtype) * torch.tensor(keep_mult(p), dtype=torch.float32).to(dtype)).view(*shape)


# ----------------------------------------------------------------------------------------- LayerNorm
def ln_case(R, seed=0, ill=False):
    """a [R, 96], b [R, 96] (the residual branch), dy [R, 96], gamma, beta, and G0 of the three accumulated column vectors.  Rows of a have
    mean 3 and standard deviation 0.5, b is a fifth of that (a + dropout(b) keeps the 0.5): the mean subtraction carries weight.  ill: row 0 of a is the constant 3 (and b's row 0 is 0), the rows
    from 8 on have a mean 1e3 times their spread (more than one of them: the ratio of two float32 evaluations of ONE row's mean is luck)."""
    g = torch.Generator().manual_seed(50021 * seed + R)
    a = 3.0 + 0.5 * torch.randn(R, D, generator=g)
    b = 0.1 * torch.randn(R, D, generator=g)
    dy = torch.randn(R, D, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    g0 = {k: torch.randn(D, generator=g) for k in ("dgamma", "dbeta", "out_colsum")}
    if ill:
        a[0] = 3.0
        b[0] = 0.0
        a[8:] = 500.0 + 0.5 * torch.randn(R - 8, D, generator=g)
    return {"R": R, "a": a, "b": b, "dy": dy, "gamma": gamma, "beta": beta, "g0": g0}


def layer_norm(x, gamma, beta, eps=LN_EPS, unbiased=False):
    """torch.nn.LayerNorm((96,)) spelled out so that the statistics can be returned: -> y, mean [R], rstd [R]"""
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=unbiased, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (x - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def ln_ref(dtype, case, p, seed, site_fwd, site_bwd, residual=True, eps=LN_EPS, unbiased=False, keep_fwd=None, keep_bwd=None):
    """pre = a + dropout(b; site_fwd) (residual) or a, y = LayerNorm(pre), stats [R, 2] = (mean, rstd); with loss sum(y * dy) under autograd:
    dx = d loss / d pre, dx_dropped = dropout(dx; site_bwd), dgamma / dbeta / out_colsum = G0 + the gradients of gamma / beta / the column
    sums of dx_dropped, out_colsum_plain = G0 + the column sums of dx (what the kernel accumulates with dx_dropped = NULL).
    keep_fwd / keep_bwd: multiplier tensors to use instead of the keep model's."""
    R = case["R"]
    a, b, dy = (case[k].to(dtype) for k in ("a", "b", "dy"))
    gamma, beta = case["gamma"].to(dtype).requires_grad_(True), case["beta"].to(dtype).requires_grad_(True)
    pre = a
    if residual:
        pre = a + b * (keep_tensor((R, D), seed, site_fwd, p, dtype) if keep_fwd is None else keep_fwd.to(dtype))
    pre = pre.detach().requires_grad_(True)
    y, mean, rstd = layer_norm(pre, gamma, beta, eps, unbiased)
    dx, dgamma, dbeta = torch.autograd.grad((y * dy).sum(), (pre, gamma, beta))
    dxd = dx * (keep_tensor((R, D), seed, site_bwd, p, dtype) if keep_bwd is None else keep_bwd.to(dtype))
    g0 = {k: v.to(dtype) for k, v in case["g0"].items()}
    return {"pre": pre.detach(), "y": y.detach(), "stats": torch.stack([mean, rstd], 1).detach(), "dx": dx, "dx_dropped": dxd,
            "dgamma": g0["dgamma"] + dgamma, "dbeta": g0["dbeta"] + dbeta, "out_colsum": g0["out_colsum"] + dxd.sum(0),
            "out_colsum_plain": g0["out_colsum"] + dx.sum(0)}


def pooled(results):
    """the results of several cases as one: every tensor flattened and concatenated under its name"""
    return {k: torch.cat([r[k].detach().reshape(-1) for r in results]) for k in results[0]}


LN_ROW_TENSORS = ("pre", "y", "stats", "dx", "dx_dropped")
LN_SUM_TENSORS = ("dgamma", "dbeta", "out_colsum", "out_colsum_plain")


@functools.lru_cache(maxsize=None)
def cached_ln_case(R, ill=False):
    return ln_case(R, ill=ill)


@functools.lru_cache(maxsize=None)
def cached_ln_ref(dtype, R, p, residual=True, ill=False):
    """shared between the tests; nobody writes into it"""
    return ln_ref(dtype, cached_ln_case(R, ill), p, SEEDS[1], SITES[0], SITES[1], residual=residual)


# ----------------------------------------------------------------------------------------- elementwise dropout and the ReLU masks
def drop_case(n, seed=0):
    """x, a second operand and relu_of [n]; relu_of carries +0.0, -0.0, negatives and a NaN at fixed places (as far as n reaches)"""
    g = torch.Generator().manual_seed(977 * seed + n)
    x, a, r = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    for pos, val in ((0, 0.0), (1, -0.0), (2, float("nan")), (3, -1.5), (n - 1, -0.0), (n // 2, float("nan"))):
        if 0 <= pos < n:
            r[pos] = val
    return {"n": n, "x": x, "a": a, "relu_of": r}


def open_gate(relu_of):
    """ReLU's gradient gate: open where relu_of > 0; +0.0, -0.0, negatives and NaN are closed"""
    return relu_of > 0


def drop_ref(dtype, case, p, seed, site, ignore_site=False):
    """dropout = x * keep, add_dropout = a + x * keep, dropout_relu = dropout gated by relu_of, relu = x gated by relu_of"""
    x, a = case["x"].to(dtype), case["a"].to(dtype)
    k = keep_tensor((case["n"],), seed, site, p, dtype, ignore_site)
    gate = open_gate(case["relu_of"]).to(dtype)
    return {"dropout": x * k, "add_dropout": a + x * k, "dropout_relu": x * k * gate, "relu": x * gate}


# ----------------------------------------------------------------------------------------- embedding of the unmasked tokens, decoder input
NPOS_EXTRA = 5          # rows of the positional table past P: the kernels must leave them alone


def embed_case(S, P, Pu, seed=0):
    """series [S, 12 P], the patch embedding w [96, 12] / b [96], pos [P + NPOS_EXTRA, 96], a random split of the P tokens into um [Pu] and
    mk [P - Pu], z [S, Pu, 96], mask_token [96], the gradients dx [S, Pu, 96] and dout [S, P, 96], and G0 of every accumulated gradient"""
    g = torch.Generator().manual_seed(7001 * seed + 131 * S + P)
    r = lambda *sh: torch.randn(*sh, generator=g)
    perm = torch.randperm(P, generator=g)
    c = {"S": S, "P": P, "Pu": Pu, "series": r(S, 12 * P), "w": r(D, 12) * 0.3, "b": r(D) * 0.1, "pos": r(P + NPOS_EXTRA, D) * 0.5,
         "um": perm[:Pu].contiguous(), "mk": perm[Pu:].contiguous(), "z": r(S, Pu, D), "mask_token": r(D) * 0.1, "dx": r(S, Pu, D),
         "dout": r(S, P, D)}
    c["g0"] = {"dpos": r(P + NPOS_EXTRA, D), "dw": r(D, 12), "db": r(D), "dmask": r(D)}
    return c


def embed_ref(dtype, c, p, seed, site, ignore_site=False):
    """x [S, Pu, 96] = sqrt(96) * dropout(W patch(s, um[t]) + b + pos[um[t]]) and, with loss sum(x * dx): dpos / dw / db = G0 + gradient"""
    S, P, Pu = c["S"], c["P"], c["Pu"]
    w, b, pos = (c[k].to(dtype).requires_grad_(True) for k in ("w", "b", "pos"))
    patches = c["series"].to(dtype).view(S, P, 12)[:, c["um"]]
    k = keep_tensor((S, Pu, D), seed, site, p, dtype, ignore_site)
    x = (patches @ w.t() + b + pos[c["um"]]) * k * torch.tensor(SQRT_D, dtype=dtype)
    dw, db, dpos = torch.autograd.grad((x * c["dx"].to(dtype)).sum(), (w, b, pos))
    g0 = c["g0"]
    return {"x": x.detach(), "dw": g0["dw"].to(dtype) + dw, "db": g0["db"].to(dtype) + db, "dpos": g0["dpos"].to(dtype) + dpos}


def dec_ref(dtype, c, p, seed, site, ignore_site=False):
    """out [S, P, 96] = sqrt(96) * (t < Pu ? z[s][t] : dropout(mask_token + pos[mk[t - Pu]])), the keep index that of `out`; with loss
    sum(out * dout): dz [S, Pu, 96], dm [S, Pm, 96] = the gradient that reaches the dropped sum (the scratch tensor of
    step_pt_dec_input_bwd), dpos / dmask = G0 + gradient"""
    S, P, Pu = c["S"], c["P"], c["Pu"]
    z, mt, pos = (c[k].to(dtype).requires_grad_(True) for k in ("z", "mask_token", "pos"))
    k = keep_tensor((S, P, D), seed, site, p, dtype, ignore_site)[:, Pu:]
    inner = (mt + pos[c["mk"]]).unsqueeze(0).expand(S, P - Pu, D)
    out = torch.cat([z, inner * k], 1) * torch.tensor(SQRT_D, dtype=dtype)
    dz, dmask, dpos, dm = torch.autograd.grad((out * c["dout"].to(dtype)).sum(), (z, mt, pos, inner))
    g0 = c["g0"]
    return {"out": out.detach(), "dz": dz, "dm": dm, "dpos": g0["dpos"].to(dtype) + dpos, "dmask": g0["dmask"].to(dtype) + dmask}


@functools.lru_cache(maxsize=None)
def cached_embed_case(S, P, Pu):
    return embed_case(S, P, Pu)


# ----------------------------------------------------------------------------------------- sums over the sequences and over rows
def seqsum_case(S, p_cnt, ldp, p_off, with_idx, seed=0):
    """dx [S, ldp, 96], idx (a random injection of the p_cnt positions into the p_cnt + NPOS_EXTRA rows of dvec) or None, G0 of dvec"""
    g = torch.Generator().manual_seed(3001 * seed + 17 * S + p_cnt + ldp + p_off)
    rows = p_cnt + NPOS_EXTRA
    return {"S": S, "p_cnt": p_cnt, "ldp": ldp, "p_off": p_off, "dx": torch.randn(S, ldp, D, generator=g),
            "idx": torch.randperm(rows, generator=g)[:p_cnt].contiguous() if with_idx else None, "g0": torch.randn(rows, D, generator=g)}


def seqsum_ref(dtype, c, skip_last_slice=False):
    """dvec[idx ? idx[j] : j] = G0 + sum_s dx[s][p_off + j].  skip_last_slice: the WRONG kernel that never visits its last slice."""
    S = c["S"] if not skip_last_slice else seq_slices(c["S"], c["p_cnt"])[-1][0]
    part = c["dx"].to(dtype)[:S, c["p_off"]:c["p_off"] + c["p_cnt"]].sum(0)
    rows = c["idx"] if c["idx"] is not None else torch.arange(c["p_cnt"])
    return c["g0"].to(dtype).index_add(0, rows, part)


def colsum_ref(dtype, x, g0):
    return g0.to(dtype) + x.to(dtype).sum(0)


# ----------------------------------------------------------------------------------------- wrong kernels (float64), for the host test
def ln_wrong(kind, case, p, seed, site_fwd, site_bwd):
    """float64 results of a LayerNorm that is wrong in one of the ways a kernel can be:
    "no_xhat_term"   dx = rstd * (dyg - mean(dyg)): the backward without the xhat * mean(dyg * xhat) term
    "eps"            eps = 1e-6
    "unbiased"       the variance divided by 95
    "stride_tail"    a strided loop that drops the last row of every second pass over the capped grid (dx row left at 0, the row missing in
                     every column sum)
    "site"           both dropout sites drawn from a stream that ignores the site"""
    f64 = torch.float64
    if kind == "eps":
        return ln_ref(f64, case, p, seed, site_fwd, site_bwd, eps=1e-6)
    if kind == "unbiased":
        return ln_ref(f64, case, p, seed, site_fwd, site_bwd, unbiased=True)
    R = case["R"]
    if kind == "site":
        return ln_ref(f64, case, p, seed, site_fwd, site_bwd, keep_fwd=keep_tensor((R, D), seed, site_fwd, p, f64, ignore_site=True),
                      keep_bwd=keep_tensor((R, D), seed, site_bwd, p, f64, ignore_site=True))
    out = dict(ln_ref(f64, case, p, seed, site_fwd, site_bwd))
    kb = keep_tensor((R, D), seed, site_bwd, p, f64)
    dy, gamma = case["dy"].to(f64), case["gamma"].to(f64)
    xhat = (out["pre"] - out["stats"][:, :1]) * out["stats"][:, 1:]
    if kind == "no_xhat_term":
        dyg = dy * gamma
        out["dx"] = out["stats"][:, 1:] * (dyg - dyg.mean(-1, keepdim=True))
        out["dx_dropped"] = out["dx"] * kb
        out["out_colsum"] = case["g0"]["out_colsum"].to(f64) + out["dx_dropped"].sum(0)
        return out
    assert kind == "stride_tail", kind
    lost = [e - 1 for i, (_, e) in enumerate(capped_strides(R)) if i % 2 == 1]
    live = torch.ones(R, 1, dtype=f64)
    live[lost] = 0.0
    out["dx"], out["dx_dropped"] = out["dx"] * live, out["dx_dropped"] * live
    out["dgamma"] = case["g0"]["dgamma"].to(f64) + (dy * xhat * live).sum(0)
    out["dbeta"] = case["g0"]["dbeta"].to(f64) + (dy * live).sum(0)
    out["out_colsum"] = case["g0"]["out_colsum"].to(f64) + out["dx_dropped"].sum(0)
    return out


def rel_l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def rule(kind):
    """(M, FLOOR) of a tensor: kind False / "row" (row-wise), True / "sum" (row-reduced), "ln" (row-reduced by the LayerNorm backward)"""
    return {False: (M_ROW, FLOOR_ROW), "row": (M_ROW, FLOOR_ROW), True: (M_SUM, FLOOR_SUM), "sum": (M_SUM, FLOOR_SUM), "ln": (M_SUM_LN, FLOOR_SUM)}[kind]


def bound(kind, e_f32):
    """the rule's right-hand side for a tensor whose float32 restatement is e_f32 from float64"""
    M, floor = rule(kind)
    return M * e_f32 + floor


assert math.isclose(SQRT_D, math.sqrt(96.0), rel_tol=1e-7)
