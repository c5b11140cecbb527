"""The training step's update half, kernel by kernel through the C ABI (step_amd/csrc/optim.hip: step_adam_clip / _sharded / _dyn,
step_dyn_advance, step_loss_fwd_bwd / step_loss_scaled_fwd_bwd / _dyn, step_scale2, step_masked_metrics) on plain tensors -- no STEP
module, no model, no graph capture -- against tests/optim_ref.py in float64, at the lengths where the grids, the float4 body and the
scalar tails meet, with misaligned parameter buffers, every hyperparameter switched on and off, labels one float32 step on either
side of the mask thresholds, NaN labels and predictions, and the reference's recorded cases.

Tolerance: the rule of tests/direct_ref.py (Compare): e_dev = err(device, f64) <= M * err(f32 reference, f64) + floor, every figure
printed as a RATIO line before anything is asserted.  The f32 reference is adam_clip_ref(float32) (bit-identical to torch.optim.Adam behind
clip_grad_norm_ on the CPU) or the CPU float32 loss / meters; it is never the device.  Adam: floor 0 (no atomics).  Loss and meters:
floor 2^-24 relative on the scalar values (one float32 rounding of an f64 sum), 0 on the gradients.  A scalar has ONE rounding error, which
can be zero: scalars (the gradient norm, the loss, the meters) are compared as the vector of their relative values dev / f64 over the
cases of a test, against the same vector of the f32 reference; lengths 1 to 5 are pooled into one tensor for the same reason.
What is exact carries no tolerance: masks, counts, zero patterns, scale2, _dyn against the eager call of the loss, a second call in the
same buffers.

The references are given the hyperparameters as the C ABI's ``float`` (optim_ref.abi_float): the device's problem is Adam with
beta2 = float32(0.999).  With the Python doubles instead (torch.optim.Adam's own arithmetic: 1 - 0.999 against 1.f - 0.999f, 1.29e-5
apart) the first run on an MI355X measured e_dev / e_f32 = 139 on v' (5.8e-6 relative with the clip off, 8.5e-7 with the gradient
clipped to a third), 5.0 on m', 2.2-3.8 on the update: the whole of it is that one constant, a property of the float ABI, not of the
kernel's arithmetic (a CPU float32 run fed the doubles is as far from the one fed the floats).

MEASURED on an MI355X, largest e_dev / e_f32:
  Adam     update 2.65 (n = 1023, t = 2, lr 3e-3, eager and _dyn alike: they were bit-identical at t = 1, 2 and 1000), 2.19 (n = 5,
           whole squared norm supplied), 1.2-1.4 elsewhere; m' 2.02 (max-abs of the 1e-12 elements), v' 1.13, out_norm 1.00;
           per element at n = 2^20 + 1 / 2^21 + 7: 0.54 / 0.06; replayed step (tests/test_gpu_graphed_step.py) 0.99.
           4 x 2.65 -> ADAM_M = 16.
  loss     loss 1.00, dpred 1.00 (identical to the f32 reference wherever the mask is), dtheta 6.67 at the threshold case (9.6, 62.6),
           2.3-3.4 at the other threshold cases, <= 2.1 elsewhere.  dtheta = coef / n * (t - y) / max(t (1 - t), 1e-12) is five float32
           roundings on the device (e_dev 3.4e-8 .. 8.5e-8), while torch's CPU backward lands at 1.0e-8 .. 2.9e-8, at or below ONE
           rounding's rms: the ratio measures the reference's luck, not a defect.  4 x 6.67 would give 32; LOSS_M stays at 16 (2.4 x the
           largest ratio; dtheta is deterministic, no atomics feed it).
  meters   MAE 0.71, RMSE 1.00, MAPE 0.54 (f64 sums, one float32 rounding: below the f32 reference's own error)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import direct_ref as D
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
ONE_SWEEP = 1 << 20          # 1024 x 256 float4 in sumsq_partial, 4096 x 256 elements in adam_clip
LENGTHS = (1, 3, 4, 5, 1023, ONE_SWEEP, ONE_SWEEP + 1, 2 * ONE_SWEEP + 7)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_tail_cases.npz")


def _L():
    from step_amd import _lib
    return _lib


def _dev(t, off=0):
    """device copy of a flat float32 tensor that starts `off` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


def _dyn_state(adam_step=0, lr=0.0, gsl_coef=0.0, seed_xor=0, reserved=0.0):
    """a hand-written 24-byte StepDynState on the device"""
    L = _L()
    h = L.StepDynState()
    h.seed_xor, h.adam_step, h.lr, h.gsl_coef, h.reserved = seed_xor, adam_step, lr, gsl_coef, reserved
    assert ctypes.sizeof(h) == 24
    return torch.frombuffer(bytearray(bytes(h)), dtype=torch.int64).clone().cuda()


def _read_dyn(t):
    L = _L()
    h = L.StepDynState()
    host = t.cpu().numpy()
    assert host.nbytes == 24
    ctypes.memmove(ctypes.addressof(h), host.ctypes.data, 24)
    return h


def run_adam(p, g, m, v, *, wd, step, max_norm, lr=HP["lr"], entry="plain", extra=None, dyn=None, off=1, g_off=0, n=None):
    """one call of step_adam_clip (entry "plain"), step_adam_clip_sharded ("sharded", extra: float or None) or step_adam_clip_dyn ("dyn",
    dyn: device StepDynState) on device copies; params / exp_avg / exp_avg_sq start `off` floats past a 16-byte boundary, the work buffer and
    out_norm start as NaN bytes.  -> host copies p', m', v', norm"""
    L = _L()
    n = p.numel() if n is None else n
    dp, dm, dv, dg = _dev(p, off), _dev(m, off), _dev(v, off), _dev(g, g_off)
    work = D._nan_floats(L.lib().step_adam_work_floats(), "cuda")
    norm = D._nan_floats(1, "cuda")
    ex = None if extra is None else torch.tensor([extra], dtype=torch.float32, device="cuda")
    b1, b2 = HP["betas"]
    st = L.stream()
    if entry == "plain":
        L.call("step_adam_clip", L.ptr(dp), L.ptr(dg), L.ptr(dm), L.ptr(dv), n, lr, b1, b2, HP["eps"], wd, step, max_norm, L.ptr(work), L.ptr(norm), st)
    elif entry == "sharded":
        L.call("step_adam_clip_sharded", L.ptr(dp), L.ptr(dg), L.ptr(dm), L.ptr(dv), n, lr, b1, b2, HP["eps"], wd, step, max_norm, L.ptr(ex),
               L.ptr(work), L.ptr(norm), st)
    else:
        L.call("step_adam_clip_dyn", L.ptr(dp), L.ptr(dg), L.ptr(dm), L.ptr(dv), n, b1, b2, HP["eps"], wd, max_norm, L.ptr(ex), L.ptr(work),
               L.ptr(norm), L.ptr(dyn), st)
    torch.cuda.synchronize()
    return dp.cpu(), dm.cpu(), dv.cpu(), norm.cpu()[0]


def refs(p, g, m, v, **kw):
    """the float64 and the float32 reference of one call, with the hyperparameters as the ABI's floats (optim_ref.abi_float)"""
    kw = {"lr": HP["lr"], "betas": HP["betas"], "eps": HP["eps"], **kw}
    kw = {k: (x if k in ("step", "extra_sumsq", "total_sumsq") else R.abi_float(x)) for k, x in kw.items()}
    return R.adam_clip_ref(torch.float64, p, g, m, v, **kw), R.adam_clip_ref(torch.float32, p, g, m, v, **kw)


def add_adam(cmp, tag, p, dev, r64, r32):
    """the UPDATE p' - p formed in float64 from the stored values (the parameter's magnitude would hide an error of the update), m', v'"""
    p64 = p.double()
    cmp.add(f"{tag} update", dev[0].double() - p64, r64[0] - p64, r32[0].double() - p64)
    cmp.add(f"{tag} m", dev[1], r64[1], r32[1])
    cmp.add(f"{tag} v", dev[2], r64[2], r32[2])


def elementwise(tag, M, p, dev_p, r64_p, r32_p):
    """max over elements of |delta| / (|update64| + ulp32(p)), device and f32 reference, under the same rule (floor 0)"""
    p64 = p.double()
    ulp = (torch.nextafter(p.abs(), torch.full_like(p, float("inf"))) - p.abs()).double()
    upd = r64_p - p64
    e_dev = float((((dev_p.double() - p64) - upd).abs() / (upd.abs() + ulp)).max())
    e_f32 = float((((r32_p.double() - p64) - upd).abs() / (upd.abs() + ulp)).max())
    print(f"RATIO {tag} elementwise max |delta| / (|update| + ulp(p)): e_dev={e_dev:.3e} e_f32={e_f32:.3e} ratio={e_dev / e_f32:8.2f}")
    assert e_dev <= M * e_f32, (tag, e_dev, e_f32)


class Scalars:
    """scalars of several cases as one tensor of relative values x / f64 (module docstring)"""

    def __init__(self):
        self.dev, self.r32 = [], []

    def add(self, dev, r64, r32):
        r64 = float(r64)
        assert r64 != 0.0
        self.dev.append(float(dev) / r64)
        self.r32.append(float(r32) / r64)

    def into(self, cmp, name, extra=0.0):
        cmp.add(name, torch.tensor(self.dev, dtype=torch.float64), torch.ones(len(self.dev), dtype=torch.float64),
                torch.tensor(self.r32, dtype=torch.float64), extra=extra)


# ================================================================================================ clip + Adam
def test_adam_lengths_with_misaligned_parameters_and_an_active_clip():
    """every length of LENGTHS: the float4 body alone, the scalar tail of block 0 alone, exactly one sweep of both grids, the grid-stride
    loops; wd and the clip on (max_norm = norm / 3), step 2; params and both moments one float past a 16-byte boundary"""
    cmp = D.Compare("adam lengths", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    norms = Scalars()
    small = {"p": [], "dev": [[], [], []], "r64": [[], [], []], "r32": [[], [], []]}
    for n in LENGTHS:
        p, g, m, v = R.adam_case(n, seed=1)
        kw = dict(wd=0.1, step=2, max_norm=float(g.double().norm()) / 3)
        r64, r32 = refs(p, g, m, v, **kw)
        dev = run_adam(p, g, m, v, **kw)
        assert float(kw["max_norm"] / (r64[3] + 1e-6)) < 0.5          # the clip is active
        norms.add(dev[3], r64[3], r32[3])
        if n <= 5:
            small["p"].append(p)
            for k in range(3):
                small["dev"][k].append(dev[k]); small["r64"][k].append(r64[k]); small["r32"][k].append(r32[k])
            continue
        add_adam(cmp, f"n={n}", p, dev, r64, r32)
        if n > ONE_SWEEP:
            elementwise(f"adam n={n}", R.ADAM_M, p, dev[0], r64[0], r32[0])
    cat = lambda xs: [torch.cat(x) for x in xs]
    add_adam(cmp, "n=1,3,4,5", torch.cat(small["p"]), cat(small["dev"]), cat(small["r64"]), cat(small["r32"]))
    norms.into(cmp, "out_norm")
    cmp.finish()


@pytest.mark.parametrize("clip", ["off", "inactive", "active"])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_hyperparameters(wd, clip):
    """every term of the update matters somewhere: weight decay on / off, the bias corrections at steps 1, 2, 1000 and 100000 (1 - beta2^t
    from 1e-3 to 1), the clip off (max_norm = 0), far above the norm and at a third of it"""
    n = 1023
    p, g, m, v = R.adam_case(n, seed=2)
    norm = float(g.double().norm())
    max_norm = {"off": 0.0, "inactive": 1e4 * norm, "active": norm / 3}[clip]
    cmp = D.Compare(f"adam wd={wd} clip={clip}", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    norms = Scalars()
    for step in (1, 2, 1000, 100000):
        kw = dict(wd=wd, step=step, max_norm=max_norm)
        r64, r32 = refs(p, g, m, v, **kw)
        dev = run_adam(p, g, m, v, **kw)
        add_adam(cmp, f"t={step}", p, dev, r64, r32)
        norms.add(dev[3], r64[3], r32[3])
    norms.into(cmp, "out_norm")
    cmp.finish()
    # the hyperparameters of this case do change the float64 answer (the comparison above is not blind to them)
    base = refs(p, g, m, v, wd=wd, step=2, max_norm=max_norm)[0][0]
    assert D.rel_l2(refs(p, g, m, v, wd=wd, step=3, max_norm=max_norm)[0][0] - p.double(), base - p.double()) > 1e-2
    base_m = refs(p, g, m, v, wd=wd, step=2, max_norm=max_norm)[0][1]
    if wd:
        assert D.rel_l2(refs(p, g, m, v, wd=0.0, step=2, max_norm=max_norm)[0][1], base_m) > 1e-3
    if clip == "active":
        assert D.rel_l2(refs(p, g, m, v, wd=wd, step=2, max_norm=0.0)[0][1], base_m) > 1e-2


def test_adam_tiny_gradients_next_to_huge_ones():
    """gradients of 1e-12 next to gradients of 1e+3 (and moments grown from such gradients): eps decides the small elements' step, the
    clip (max_norm 3 against a norm of ~3e4) the large ones'"""
    n = 4099
    scale = torch.where(torch.arange(n) % 2 == 0, torch.tensor(1e-12), torch.tensor(1e3))
    p, g, m, v = R.adam_case(n, seed=3, gscale=scale)
    kw = dict(wd=0.0, step=3, max_norm=3.0)          # (weight decay would put 0.1 p ~ 1e-2 on top of the 1e-12 gradients)
    r64, r32 = refs(p, g, m, v, **kw)
    dev = run_adam(p, g, m, v, **kw)
    cmp = D.Compare("adam 1e-12 / 1e+3", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    for name, sel in (("small", slice(0, None, 2)), ("large", slice(1, None, 2))):
        add_adam(cmp, name, p[sel], [t[sel] for t in dev[:3]], [t[sel] for t in r64[:3]], [t[sel] for t in r32[:3]])
    s = Scalars()
    s.add(dev[3], r64[3], r32[3])
    s.into(cmp, "out_norm", extra=2.0 ** -24)          # one scalar: its own float32 rounding
    cmp.finish()
    small = (r64[0] - p.double())[0::2].abs()
    no_eps = refs(p, g, m, v, eps=0.0, **kw)[0][0]
    assert D.rel_l2((no_eps - p.double())[0::2], (r64[0] - p.double())[0::2]) > 0.5 and float(small.max()) > 0          # eps acts


def test_adam_sharded_norm_modes():
    """extra_sumsq is ADDED to the buffer's own sum of squares; max_norm < 0 means extra_sumsq IS the whole squared norm, clipped at
    -max_norm.  Both with a value that differs from the buffer's own sum.  out_norm is what adam_clip_kernel writes: the square root of the
    sum the clip coefficient was formed from."""
    cmp = D.Compare("adam sharded", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    norms = Scalars()
    for n in (5, 1023, ONE_SWEEP + 1):
        p, g, m, v = R.adam_case(n, seed=4)
        own = float((g.double() ** 2).sum())
        extra = float(np.float32(2.5 * own))
        for mode in ("extra", "total", "null"):
            kw = dict(wd=0.1, step=2, max_norm=own ** 0.5 / 3)
            if mode == "extra":
                r64, r32 = refs(p, g, m, v, extra_sumsq=extra, **kw)
                dev = run_adam(p, g, m, v, entry="sharded", extra=extra, **kw)
                want64, want32 = (r64[3] ** 2 + extra).sqrt(), (r32[3] * r32[3] + torch.tensor(extra)).sqrt()
            elif mode == "total":
                r64, r32 = refs(p, g, m, v, total_sumsq=extra, **kw)
                dev = run_adam(p, g, m, v, entry="sharded", extra=extra, **{**kw, "max_norm": -kw["max_norm"]})
                want64, want32 = torch.tensor(extra, dtype=torch.float64).sqrt(), torch.tensor(extra).sqrt()
            else:          # extra_sumsq = NULL through the sharded entry point: the plain call
                r64, r32 = refs(p, g, m, v, **kw)
                dev = run_adam(p, g, m, v, entry="sharded", extra=None, **kw)
                want64, want32 = r64[3], r32[3]
            add_adam(cmp, f"n={n} {mode}", p, dev, r64, r32)
            norms.add(dev[3], want64, want32)
        # the three modes are three different updates
        a, b, c = (refs(p, g, m, v, **k2, wd=0.1, step=2, max_norm=own ** 0.5 / 3)[0][1] for k2 in ({}, {"extra_sumsq": extra}, {"total_sumsq": extra}))
        assert D.rel_l2(a, b) > 1e-3 and D.rel_l2(b, c) > 1e-3
    norms.into(cmp, "out_norm")
    cmp.finish()


def test_adam_refuses_bad_arguments_before_any_launch():
    """error returns (STEP_REQUIRE on the host, nothing is launched): the text of step_last_error through _lib.check, buffers untouched"""
    p, g, m, v = R.adam_case(64, seed=5)
    ok = dict(wd=0.0, step=1, max_norm=1.0)
    with pytest.raises(RuntimeError, match="gradient buffer must be 16-byte aligned"):
        run_adam(p, g, m, v, g_off=1, **ok)
    with pytest.raises(RuntimeError, match="needs extra_sumsq"):
        run_adam(p, g, m, v, entry="sharded", extra=None, **{**ok, "max_norm": -1.0})
    with pytest.raises(RuntimeError, match="bad arguments"):
        run_adam(p, g, m, v, **{**ok, "step": 0})
    with pytest.raises(RuntimeError, match="bad arguments"):
        run_adam(p, g, m, v, n=0, **ok)
    with pytest.raises(RuntimeError, match="null state"):
        run_adam(p, g, m, v, entry="dyn", dyn=None, wd=0.0, step=1, max_norm=1.0)
    dev = run_adam(p, g, m, v, **ok)          # and the library still works
    assert torch.isfinite(dev[0]).all() and not torch.equal(dev[0], p)


def test_adam_five_chained_steps():
    """five steps in the same device buffers with fresh gradients; after each one p, m, v against one reference step from the state the
    device held before it (what step t wrote is what step t + 1 reads), and the final parameters against five chained reference steps"""
    L = _L()
    n = 4099
    p, g, m, v = R.adam_case(n, seed=6)
    gen = torch.Generator().manual_seed(66)
    dp, dm, dv = _dev(p, 1), _dev(m, 1), _dev(v, 1)
    work, norm = D._nan_floats(L.lib().step_adam_work_floats(), "cuda"), D._nan_floats(1, "cuda")
    cmp = D.Compare("adam chained", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    c64, c32 = (p.double(), m.double(), v.double()), (p, m, v)
    for t in range(3, 8):
        g = torch.randn(n, generator=gen) * (0.5 + t)
        kw = dict(wd=0.01, step=t, max_norm=40.0)
        before = (dp.cpu(), dm.cpu(), dv.cpu())
        L.call("step_adam_clip", L.ptr(dp), L.ptr(_dev(g)), L.ptr(dm), L.ptr(dv), n, HP["lr"], *HP["betas"], HP["eps"], kw["wd"], t, kw["max_norm"],
               L.ptr(work), L.ptr(norm), L.stream())
        torch.cuda.synchronize()
        r64, r32 = refs(*before[:1], g, *before[1:], **kw)
        add_adam(cmp, f"t={t}", before[0], (dp.cpu(), dm.cpu(), dv.cpu()), r64, r32)
        c64 = refs(c64[0], g, c64[1], c64[2], **kw)[0][:3]
        c32 = refs(c32[0], g, c32[1], c32[2], **kw)[1][:3]
    add_adam(cmp, "after 5", p, (dp.cpu(), dm.cpu(), dv.cpu()), c64, c32)
    cmp.finish()


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_dyn_reads_step_count_and_learning_rate_from_the_device(t):
    """step_adam_clip_dyn with a hand-written StepDynState {adam_step = t, lr} against the float64 reference at (t, lr), next to the
    eager call step_adam_clip_sharded(step = t, lr).  Not asserted bit-identical: the eager call forms 1 - beta^t with the host's powf,
    the replayed one with the device's.  A step count off by one moves the update by tens of percent at t = 1 and 2 and by 0.03 % at
    t = 1000; the last line shows that this is ten times what the rule allows."""
    n = 1023
    lr = 3e-3
    p, g, m, v = R.adam_case(n, seed=7)
    kw = dict(wd=0.1, max_norm=float(g.double().norm()) / 3)
    extra = float(np.float32(0.5 * float((g.double() ** 2).sum())))
    dyn = _dyn_state(adam_step=t, lr=lr, gsl_coef=123.0, seed_xor=77, reserved=5.0)
    got = run_adam(p, g, m, v, entry="dyn", dyn=dyn, extra=extra, step=None, **kw)
    eager = run_adam(p, g, m, v, entry="sharded", extra=extra, step=t, lr=lr, **kw)
    r64, r32 = refs(p, g, m, v, step=t, lr=lr, extra_sumsq=extra, **kw)
    cmp = D.Compare(f"adam dyn t={t}", R.ADAM_M, R.ADAM_FLOOR, 0.0)
    add_adam(cmp, "dyn", p, got, r64, r32)
    add_adam(cmp, "eager", p, eager, r64, r32)
    print(f"RATIO adam dyn t={t}: bit-identical to the eager call: p {torch.equal(got[0], eager[0])} m {torch.equal(got[1], eager[1])} "
          f"v {torch.equal(got[2], eager[2])}")
    assert torch.equal(got[1], eager[1]) and torch.equal(got[2], eager[2]) and torch.equal(got[3], eager[3])          # no bias correction in these
    cmp.finish()
    h = _read_dyn(dyn)          # read only
    assert (h.seed_xor, h.adam_step, h.gsl_coef, h.reserved) == (77, t, 123.0, 5.0) and h.lr == float(np.float32(lr))
    off_by_one = refs(p, g, m, v, step=t + 1, lr=lr, extra_sumsq=extra, **kw)[0][0]
    assert D.rel_l2(off_by_one - p.double(), r64[0] - p.double()) > 10 * R.ADAM_M * D.rel_l2(r32[0].double() - p.double(), r64[0] - p.double())


def test_dyn_advance():
    """applied 3 times: adam_step + 3, seed_xor = splitmix64 iterated, lr / gsl_coef / reserved untouched"""
    L = _L()
    seed = 0xD1B54A32D192ED03
    dyn = _dyn_state(adam_step=41, lr=2e-3, gsl_coef=0.25, seed_xor=seed, reserved=-7.5)
    want = seed
    for k in range(3):
        L.call("step_dyn_advance", L.ptr(dyn), L.stream())
        want = R.splitmix64(want)
        torch.cuda.synchronize()
        h = _read_dyn(dyn)
        assert h.seed_xor == want and h.adam_step == 42 + k
    assert (h.lr, h.gsl_coef, h.reserved) == (float(np.float32(2e-3)), 0.25, -7.5)
    with pytest.raises(RuntimeError, match="null state"):
        L.call("step_dyn_advance", None, L.stream())


def test_adam_two_runs_are_identical():
    """no atomics anywhere in the two kernels: the same inputs give the same bits"""
    n = LENGTHS[-1]
    p, g, m, v = R.adam_case(n, seed=8)
    kw = dict(wd=0.1, step=5, max_norm=float(g.double().norm()) / 3)
    a, b = run_adam(p, g, m, v, **kw), run_adam(p, g, m, v, off=3, **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ================================================================================================ loss
def run_loss(pred, real, rs, theta, prior, coef, null_val=0.0, scale=1.0, shift=0.0, entry="scaled"):
    """step_loss_fwd_bwd ("plain": scale 1, shift 0, stride 1), step_loss_scaled_fwd_bwd ("scaled") or step_loss_scaled_fwd_bwd_dyn ("dyn":
    coef is a device StepDynState) on flat device copies; real: the strided buffer [n_pred * rs].  Outputs and work start as NaN bytes.
    -> loss, dpred, dtheta (host), work (3 doubles after the call: S_abs, count, S_bce)"""
    L = _L()
    n_pred, n_adj = pred.numel(), theta.numel()
    assert real.numel() == n_pred * rs and prior.numel() == n_adj
    dp, dr, dt, da = (x.reshape(-1).contiguous().cuda() for x in (pred, real, theta, prior))
    loss, dpred, dtheta = D._nan_floats(1, "cuda"), D._nan_floats(n_pred, "cuda"), D._nan_floats(n_adj, "cuda")
    work = D._nan_floats(6, "cuda").view(torch.float64)
    st = L.stream()
    if entry == "plain":
        assert rs == 1 and scale == 1.0 and shift == 0.0
        L.call("step_loss_fwd_bwd", L.ptr(dp), L.ptr(dr), n_pred, L.ptr(dt), L.ptr(da), n_adj, null_val, coef, L.ptr(work), L.ptr(loss), L.ptr(dpred),
               L.ptr(dtheta), st)
    elif entry == "scaled":
        L.call("step_loss_scaled_fwd_bwd", L.ptr(dp), L.ptr(dr), n_pred, rs, scale, shift, L.ptr(dt), L.ptr(da), n_adj, null_val, coef, L.ptr(work),
               L.ptr(loss), L.ptr(dpred), L.ptr(dtheta), st)
    else:
        L.call("step_loss_scaled_fwd_bwd_dyn", L.ptr(dp), L.ptr(dr), n_pred, rs, scale, shift, L.ptr(dt), L.ptr(da), n_adj, null_val, L.ptr(work),
               L.ptr(loss), L.ptr(dpred), L.ptr(dtheta), L.ptr(coef), st)
    torch.cuda.synchronize()
    return loss.cpu()[0], dpred.cpu(), dtheta.cpu(), work.cpu()


def loss_case(n_pred, n_adj, rs, seed, std=150.0, mean=200.0):
    g = torch.Generator().manual_seed(seed * 7919 + n_pred + 3 * n_adj + rs)
    real = torch.randn(n_pred * rs, generator=g)
    lab = real[::rs]
    lab[torch.rand(n_pred, generator=g) < 0.15] = float(np.float32(-mean / std))          # rescales to (about) the null value
    pred = lab + 0.1 * torch.randn(n_pred, generator=g)
    theta = torch.rand(n_adj, generator=g).clamp(1e-4, 1 - 1e-4)
    prior = (torch.rand(n_adj, generator=g) < 0.2).float()
    return pred, real, theta, prior


def add_loss(cmp, scal, tag, got, r64, r32):
    """the exact part (mask as dpred's zero pattern, count) asserted here; loss into `scal`; both gradients into `cmp`"""
    loss, dpred, dtheta, work = got
    mask = r64["mask"].reshape(-1)
    assert torch.equal(dpred != 0, mask), f"{tag}: {int(((dpred != 0) != mask).sum())} labels with another mask than the reference's"
    assert float(work[1]) == r64["count"], (tag, float(work[1]), r64["count"])
    if r64["count"]:          # the denominator, once more from the gradient itself: |dpred| = scale / count on an unmasked element
        assert bool(torch.isfinite(loss))
    scal.add(loss, r64["loss"], r32["loss"])
    if r64["count"]:
        cmp.add(f"{tag} dpred", dpred, r64["dpred"].reshape(-1), r32["dpred"].reshape(-1))
    else:
        assert float(dpred.abs().max()) == 0.0
    cmp.add(f"{tag} dtheta", dtheta, r64["dtheta"].reshape(-1), r32["dtheta"].reshape(-1))


LOSS_SIZES = [(1, 1), (255, 4), (12 * 37, 37 * 37), (4096 * 3 + 5, 130 * 130), (130 * 130, 4096 * 3 + 5)]


@pytest.mark.parametrize("rs", [1, 3])
def test_loss_sizes(rs):
    """one element, fewer elements than a block, the size of the golden model, several reduce blocks with n_adj > n_pred, and the
    reverse; the label read in place with stride rs; step_loss_fwd_bwd (rs = 1) agrees bit for bit with the scaled entry at scale 1"""
    std, mean, coef = 150.0, 200.0, 0.7
    cmp = D.Compare(f"loss rs={rs}", R.LOSS_M, 0.0, 0.0)
    scal = Scalars()
    for n_pred, n_adj in LOSS_SIZES:
        pred, real, theta, prior = loss_case(n_pred, n_adj, rs, seed=1)
        lab = real[::rs].contiguous()
        if n_pred == 1:
            lab[0] = real[0] = 0.25          # (the one label must not be the masked one)
            pred = lab + 0.1
        r64, r32 = (R.loss_ref(dt, pred, lab, theta, prior, coef, 0.0, std, mean) for dt in (torch.float64, torch.float32))
        got = run_loss(pred, real, rs, theta, prior, coef, 0.0, std, mean)
        add_loss(cmp, scal, f"{n_pred}/{n_adj}", got, r64, r32)
        if rs == 1:
            y = R.torch_rescale(lab, std, mean)
            p = R.torch_rescale(pred, std, mean)
            a = run_loss(p, y, 1, theta, prior, coef, 0.0, entry="plain")
            b = run_loss(p, y, 1, theta, prior, coef, 0.0, 1.0, 0.0, entry="scaled")
            assert all(torch.equal(x, z) for x, z in zip(a, b))
            assert torch.equal(a[1] != 0, r64["mask"].reshape(-1)) and float(a[3][1]) == r64["count"]
    scal.into(cmp, "loss", extra=R.LOSS_FLOOR)
    cmp.finish()


@pytest.mark.parametrize("std,mean", R.SCALERS)
def test_loss_mask_at_the_threshold(std, mean):
    """labels within 400 float32 steps of -mean / std, in channel 0 of a [B, 12, N, C] batch tensor: after the rescale they sit one
    float32 step apart on both sides of the 5e-5 threshold.  The zero pattern of dpred must be the mask of torch's float32
    ``y * std + mean`` EXACTLY, and the loss's denominator its count: a rescale rounded once flips 1 or 2 of these labels for every scaler
    but the control (150, 200) (tests/test_optim_ref_host.py)."""
    B, N, C = 2, 37, 3
    g = torch.Generator().manual_seed(int(std * 10))
    lab = R.threshold_labels(std, mean)
    n = B * 12 * N
    lab = lab[torch.arange(n) % lab.numel()]
    real = torch.randn(B, 12, N, C, generator=g)
    real[..., 0] = lab.view(B, 12, N)
    pred = lab + 0.1 * (0.5 + torch.rand(n, generator=g)) * (1 - 2 * (torch.arange(n) % 2))          # label + noise, never equal to it
    theta = torch.rand(B * N * N, generator=g).clamp(1e-4, 1 - 1e-4)
    prior = (torch.rand(B * N * N, generator=g) < 0.2).float()
    r64, r32 = (R.loss_ref(dt, pred, lab, theta, prior, 0.5, 0.0, std, mean) for dt in (torch.float64, torch.float32))
    fused = R.mae_mask(R.fused_rescale(lab, std, mean), 0.0)
    print(f"RATIO threshold ({std}, {mean}): {n} labels, {n - r64['count']} masked, a rescale rounded once would flip {int((fused != r64['mask']).sum())}")
    assert 0 < r64["count"] < n
    got = run_loss(pred, real.reshape(-1), C, theta, prior, 0.5, 0.0, std, mean)
    flips = int(((got[1] != 0) != r64["mask"]).sum())
    print(f"RATIO threshold ({std}, {mean}): device mask differs on {flips} labels, device count {float(got[3][1]):.0f}, reference count {r64['count']}")
    cmp = D.Compare(f"loss threshold ({std}, {mean})", R.LOSS_M, 0.0, 0.0)
    scal = Scalars()
    add_loss(cmp, scal, "thr", got, r64, r32)
    # the count once more, from the gradient itself: |dpred| = std / count on every unmasked element
    mag = got[1][r64["mask"]].abs()
    assert float(mag.min()) == float(mag.max()) and round(float(np.float32(std)) / float(mag[0])) == r64["count"]
    scal.into(cmp, "loss", extra=R.LOSS_FLOOR)
    cmp.finish()
    # ... and through the autograd wrapper, the label as a strided view of the batch tensor
    from step_amd.step_loss import step_loss_native
    pd = pred.view(B, 12, N, 1).cuda().requires_grad_(True)
    td = theta.view(B, N, N).cuda().requires_grad_(True)
    loss = step_loss_native(pd, real.cuda()[..., :1], td, prior.view(B, N, N).cuda(), 0.5, null_val=0.0, rescale=(mean, std))
    dp, dt = torch.autograd.grad(loss, [pd, td])
    assert torch.equal(loss.detach().cpu(), got[0]) and torch.equal(dp.cpu().reshape(-1), got[1]) and torch.equal(dt.cpu().reshape(-1), got[2])
    # ... and masked_mae_native (the pre-training loss): the same two launches with a one-edge graph term of coefficient 0
    from step_amd.step_loss import masked_mae_native
    mae = masked_mae_native(pd, real.cuda()[..., :1], 0.0, rescale=(mean, std))
    half = torch.full((1,), 0.5)
    alone = run_loss(pred, real.reshape(-1), C, half, half, 0.0, 0.0, std, mean)
    assert torch.equal(mae.detach().cpu(), alone[0]) and torch.equal(torch.autograd.grad(mae, pd)[0].cpu().reshape(-1), got[1])
    assert float(alone[3][1]) == r64["count"]


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("c", ["a", "b", "c", "d", "e0", "e11"])
def test_loss_and_meters_on_the_recorded_reference_cases(c):
    """tests/golden/train_tail_cases.npz at k = 12 through step_loss_native(..., rescale=...) and masked_metrics_native on the rescaled
    tensors, against the reference's recorded loss, metrics, dpred and dtheta; tolerances of tests/test_gpu_train_tail.py: loss rel 1e-5,
    gradients rel_l2 1e-5, metrics rtol 2e-5 / atol 1e-6.  e0 / e11 hold one NaN prediction at an unmasked label: the reference's loss is
    finite (nan_to_num) and that prediction's gradient is 0."""
    from step_amd.step_loss import masked_metrics_native, step_loss_native
    from tests.helpers import rel_l2
    z = fixture()
    mean, std = float(z[f"{c}.shift"]), float(z[f"{c}.scale"])
    pred = torch.from_numpy(z[f"{c}.pred"])[..., None].cuda().requires_grad_(True)
    theta = torch.from_numpy(z[f"{c}.theta"]).cuda().requires_grad_(True)
    real = torch.from_numpy(z[f"{c}.real"]).cuda()[..., :1]
    prior = torch.from_numpy(z[f"{c}.prior"]).cuda()
    loss = step_loss_native(pred, real, theta, prior, float(z[f"{c}.coef"]), null_val=0.0, rescale=(mean, std))
    dp, dt = torch.autograd.grad(loss, [pred, theta])
    metrics = masked_metrics_native(pred.detach() * std + mean, real * std + mean, 0.0).cpu()
    dp, dt = dp[..., 0].cpu(), dt.cpu()
    print(c, "loss", float(loss), float(z[f"{c}.12.loss"]), "metrics", metrics.tolist(), z[f"{c}.12.metrics"].tolist())
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dp).all()) and bool(torch.isfinite(metrics).all())
    assert float(loss) == pytest.approx(float(z[f"{c}.12.loss"]), rel=1e-5)
    assert torch.allclose(metrics, torch.from_numpy(z[f"{c}.12.metrics"]), rtol=2e-5, atol=1e-6)
    assert rel_l2(dt, torch.from_numpy(z[f"{c}.dtheta"])) < 1e-5
    y = torch.from_numpy(z[f"{c}.real"][..., 0]) * std + mean
    assert torch.equal(dp != 0, R.mae_mask(y, 0.0) & ~torch.isnan(torch.from_numpy(z[f"{c}.pred"])))
    if f"{c}.12.dpred" in z:
        assert rel_l2(dp, torch.from_numpy(z[f"{c}.12.dpred"])) < 1e-5
    else:
        nan_at = torch.isnan(torch.from_numpy(z[f"{c}.pred"]))
        assert c in ("e0", "e11") and int(nan_at.sum()) == 1 and bool((dp[nan_at] == 0).all())


def test_loss_nan_labels_and_predictions():
    """a NaN label is not close to a finite null value: it counts in the denominator and adds 0 (where(isnan(loss), 0, loss)); so does a
    NaN prediction at an unmasked label; both have gradient 0.  Reference: the CPU functions."""
    std, mean = 150.0, 200.0
    for rs, null in ((1, 0.0), (3, 0.0), (1, 200.0)):
        pred, real, theta, prior = loss_case(500, 49, rs, seed=2, std=std, mean=mean if null == 0.0 else 0.0)
        lab = real[::rs]
        lab[7] = lab[300] = float("nan")
        pred = pred.clone()
        pred[7] = 0.3          # (it was label + noise: NaN)
        pred[300] = 0.1
        pred[11] = float("nan")
        lab = lab.contiguous()
        r64, r32 = (R.loss_ref(dt, pred, lab, theta, prior, 1.0, null, std, mean) for dt in (torch.float64, torch.float32))
        assert bool(r64["mask"][7]) and bool(r64["mask"][300]) and bool(r64["mask"][11])
        got = run_loss(pred, real, rs, theta, prior, 1.0, null, std, mean)
        print(f"RATIO nan rs={rs} null={null}: device loss {float(got[0])}, reference {float(r64['loss'])}; device count {float(got[3][1]):.0f}, "
              f"reference {r64['count']}; dpred at the NaNs {got[1][[7, 300, 11]].tolist()}")
        assert bool(torch.isfinite(got[0])) and float(got[3][1]) == r64["count"]
        assert got[1][[7, 300, 11]].tolist() == [0.0, 0.0, 0.0]
        expect = r64["mask"].clone()
        expect[[7, 300, 11]] = False          # counted, but their own gradient is 0
        assert torch.equal(got[1] != 0, expect)
        cmp = D.Compare(f"loss nan rs={rs} null={null}", R.LOSS_M, 0.0, 0.0)
        scal = Scalars()
        scal.add(got[0], r64["loss"], r32["loss"])
        cmp.add("dpred", got[1], r64["dpred"], r32["dpred"])
        cmp.add("dtheta", got[2], r64["dtheta"], r32["dtheta"])
        scal.into(cmp, "loss", extra=R.LOSS_FLOOR)
        cmp.finish()


def test_loss_all_masked_batch():
    """every label at the null value: the loss is the graph term alone, dpred all zero, count 0"""
    for n_pred in (1, 5000):
        pred, _, theta, prior = loss_case(n_pred, 300, 1, seed=3)
        real = torch.full((n_pred,), float(np.float32(-200.0 / 150.0)))
        r64, r32 = (R.loss_ref(dt, pred, real, theta, prior, 0.5, 0.0, 150.0, 200.0) for dt in (torch.float64, torch.float32))
        assert r64["count"] == 0
        got = run_loss(pred, real, 1, theta, prior, 0.5, 0.0, 150.0, 200.0)
        assert float(got[3][1]) == 0.0 and float(got[1].abs().max()) == 0.0 and float(got[0]) > 0
        cmp = D.Compare(f"loss all masked n={n_pred}", R.LOSS_M, 0.0, 0.0)
        scal = Scalars()
        add_loss(cmp, scal, "masked", got, r64, r32)
        scal.into(cmp, "loss", extra=R.LOSS_FLOOR)
        cmp.finish()


def test_loss_graph_term_edges():
    """theta exactly 0 and exactly 1 with a prior of both values (torch's -100 clamp of the logs, the 1e-12 floor of the backward's
    denominator), theta at 1e-7 and at 1 - 6e-8, among ordinary values"""
    g = torch.Generator().manual_seed(9)
    n_adj = 1000
    theta = torch.rand(n_adj, generator=g).clamp(1e-4, 1 - 1e-4)
    prior = (torch.rand(n_adj, generator=g) < 0.3).float()
    edge = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (1e-7, 0.0), (1e-7, 1.0), (1 - 6e-8, 0.0), (1 - 6e-8, 1.0)]
    for i, (t, y) in enumerate(edge):
        theta[17 * i + 3], prior[17 * i + 3] = t, y
    assert float(theta[17 * 6 + 3]) < 1.0
    pred, real, _, _ = loss_case(255, 4, 1, seed=4)
    r64, r32 = (R.loss_ref(dt, pred, real, theta, prior, 0.7, 0.0, 150.0, 200.0) for dt in (torch.float64, torch.float32))
    got = run_loss(pred, real, 1, theta, prior, 0.7, 0.0, 150.0, 200.0)
    cmp = D.Compare("loss graph edges", R.LOSS_M, 0.0, 0.0)
    scal = Scalars()
    add_loss(cmp, scal, "edges", got, r64, r32)
    idx = torch.tensor([17 * i + 3 for i in range(len(edge))])
    cmp.add("dtheta at the edges", got[2][idx], r64["dtheta"].reshape(-1)[idx], r32["dtheta"].reshape(-1)[idx])
    scal.into(cmp, "loss", extra=R.LOSS_FLOOR)
    cmp.finish()
    assert float(r64["loss"]) > 0.7 * 200.0 / n_adj          # the two clamped logs (100 each) are in the mean


def test_loss_dyn_reads_the_coefficient_from_the_device():
    """step_loss_scaled_fwd_bwd_dyn: gsl_coef comes from the struct; bit for bit the eager call with that coefficient"""
    pred, real, theta, prior = loss_case(12 * 37, 37 * 37, 3, seed=5)
    coef = float(np.float32(0.37))
    dyn = _dyn_state(adam_step=9, lr=1.0, gsl_coef=coef, seed_xor=1, reserved=2.0)
    a = run_loss(pred, real, 3, theta, prior, dyn, 0.0, 150.0, 200.0, entry="dyn")
    b = run_loss(pred, real, 3, theta, prior, coef, 0.0, 150.0, 200.0)
    c = run_loss(pred, real, 3, theta, prior, 1.0, 0.0, 150.0, 200.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    h = _read_dyn(dyn)
    assert (h.seed_xor, h.adam_step, h.lr, h.gsl_coef, h.reserved) == (1, 9, 1.0, coef, 2.0)


@pytest.mark.parametrize("na,nb", [(300001, 257), (257, 300001), (1, 3)])
def test_scale2(na, nb):
    """out_a = a * g, out_b = b * g with g a device scalar: na != nb, both with tails, either one the larger (and beyond one sweep of the
    grid of 1024 x 256); bit for bit"""
    L = _L()
    gen = torch.Generator().manual_seed(na)
    a, b = torch.randn(na, generator=gen).cuda(), torch.randn(nb, generator=gen).cuda()
    g = torch.tensor([0.37], device="cuda")
    oa, ob = D._nan_floats(na, "cuda"), D._nan_floats(nb, "cuda")
    L.call("step_scale2", L.ptr(a), na, L.ptr(b), nb, L.ptr(g), L.ptr(oa), L.ptr(ob), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(oa, a * g) and torch.equal(ob, b * g)


# ================================================================================================ the three meters
def run_metrics(pred, ps, real, rs, n, null_val, work=None):
    L = _L()
    dp, dr = pred.contiguous().cuda(), real.contiguous().cuda()
    assert dp.numel() == n * ps and dr.numel() == n * rs
    work = torch.zeros(6, dtype=torch.float64, device="cuda") if work is None else work
    out = D._nan_floats(3, "cuda")
    L.call("step_masked_metrics", L.ptr(dp), ps, L.ptr(dr), rs, n, null_val, L.ptr(work), L.ptr(out), L.stream())
    torch.cuda.synchronize()
    return out.cpu(), work


def threshold_values(null):
    """float32(5e-5) and float32(1e-4) exactly and one step either side of each, both signs, offset by the null value"""
    out = []
    for v in (5e-5, 1e-4):
        t = torch.tensor(v, dtype=torch.float32)
        out += [t, torch.nextafter(t, torch.tensor(1.0)), torch.nextafter(t, torch.tensor(0.0))]
    vals = torch.stack(out)
    return torch.cat([vals, -vals]) + null


@pytest.mark.parametrize("null", [0.0, -1.0])
def test_masked_metrics(null):
    """n = 1, one block with a tail, three blocks, the block cap of 256 with a grid-stride loop; prediction and label both strided;
    labels given already rescaled: exactly at, and one float32 step either side of, this kernel's own thresholds (5e-5 around the null
    value, 1e-4 and 5e-5 around 0 for MAPE); a NaN label and a NaN prediction; a second call on the same work buffer gives the same bits"""
    ps, rs = 2, 3
    cmp = D.Compare(f"metrics null={null}", R.LOSS_M, 0.0, 0.0)
    scal = [Scalars(), Scalars(), Scalars()]
    for n in (1, 4095, 4096 * 2 + 1, 4096 * 300):
        gen = torch.Generator().manual_seed(n)
        real = torch.randn(n * rs, generator=gen) * 50 + 100
        pred = torch.randn(n * ps, generator=gen) * 50 + 100
        lab, p = real[::rs], pred[::ps]
        if n > 1:
            lab[torch.rand(n, generator=gen) < 0.2] = null
            thr = torch.cat([threshold_values(null), threshold_values(0.0)])
            lab[100:100 + thr.numel()] = thr
            lab[50] = float("nan")
            p[60] = float("nan")
        p[:] = torch.where(torch.isnan(p), p, lab + torch.randn(n, generator=gen) * 10)
        if n > 1:
            p[50] = 3.0
        lab, p = lab.contiguous(), p.contiguous()
        r64, r32 = R.masked_metrics_ref(p, lab, null, dtype=torch.float64), R.masked_metrics_ref(p, lab, null)
        got, work = run_metrics(pred, ps, real, rs, n, null)
        again, _ = run_metrics(pred, ps, real, rs, n, null, work=work)
        print(f"RATIO metrics null={null} n={n}: device {got.tolist()} float64 {r64.tolist()}")
        assert torch.equal(got, again) and bool((work == 0).all())          # the buffer was left clean
        assert bool(torch.isfinite(got).all())
        for k in range(3):
            if float(r64[k]) == 0.0:
                assert float(got[k]) == 0.0
            else:
                scal[k].add(got[k], r64[k], r32[k])
    for k, name in enumerate(("MAE", "RMSE", "MAPE")):
        scal[k].into(cmp, name, extra=R.LOSS_FLOOR)
    cmp.finish()


def test_masked_metrics_mask_counts_at_the_thresholds():
    """the twelve threshold labels alone, one call each: whether the label counts for MAE (|y - null| <= float32(5e-5) does not) and for
    MAPE (|y| < float32(1e-4) does not) is read off the result being zero or not -- exact, no tolerance"""
    for null in (0.0, -1.0):
        for y in torch.cat([threshold_values(null), threshold_values(0.0)]).tolist():
            lab = torch.tensor([y], dtype=torch.float32)
            p = lab + 2.0
            want = R.masked_metrics_ref(p, lab, null, dtype=torch.float64)
            got, _ = run_metrics(p, 1, lab, 1, 1, null)
            assert [float(v) != 0.0 for v in got] == [float(v) != 0.0 for v in want], (null, y, got.tolist(), want.tolist())
