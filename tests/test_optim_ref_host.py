"""tests/optim_ref.py against what it restates, on the CPU: the Adam + clip reference against torch.optim.Adam behind
clip_grad_norm_, the loss and the meters against oracle.step_oracle / step_amd.step_loss, splitmix64 against published vectors -- and the
condition that keeps the threshold cases of tests/test_gpu_optim_direct.py from being vacuous: the labels they use must get a different
mask from a rescale rounded once than from torch's, for the scalers that are there to show it, and the same mask for the control."""
import numpy as np
import pytest
import torch

from oracle import step_oracle as O
from tests import optim_ref as R


def _torch_adam_run(dtype, p0, grads, *, lr, betas, eps, wd, max_norm):
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    out = []
    for g in grads:
        p.grad = g.to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm=max_norm, foreach=False) if max_norm else torch.linalg.vector_norm(p.grad)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), norm.detach().clone()))
    return out


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("clip", ["active", "inactive", "off"])
def test_adam_reference_is_torch_adam_behind_clip_grad_norm(wd, clip):
    """float64: 1e-12 relative over 5 steps.  float32: BIT FOR BIT -- adam_clip_ref uses torch's own operation order (lerp_, addcmul_,
    addcdiv_, the bias corrections as Python floats), so there is no 1-ulp allowance to make."""
    n = 1000
    gen = torch.Generator().manual_seed(11)
    p0 = 0.1 * torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(5)]
    norm0 = float(grads[0].norm())
    max_norm = {"active": norm0 / 3, "inactive": norm0 * 100, "off": 0.0}[clip]
    hp = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=wd)
    for dtype in (torch.float64, torch.float32):
        want = _torch_adam_run(dtype, p0, grads, max_norm=max_norm, **hp)
        p, m, v = p0.to(dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
        for t, g in enumerate(grads, 1):
            before = p
            p, m, v, norm = R.adam_clip_ref(dtype, p, g, m, v, step=t, max_norm=max_norm, **hp)
            assert p.dtype == dtype and not torch.equal(p, before)
            for got, ref in zip((p, m, v, norm), want[t - 1]):
                if dtype == torch.float32:
                    assert torch.equal(got, ref), (clip, wd, t)
                else:
                    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (clip, wd, t)
    # the clip did what the case's name says
    coef = max_norm / (norm0 + 1e-6) if max_norm else 1.0
    assert (coef < 1.0) == (clip == "active")


def test_adam_reference_norm_modes():
    gen = torch.Generator().manual_seed(12)
    n = 257
    p, g, m, v = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(4))
    v = v.abs()
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, step=3, max_norm=1.0)
    own = float((g * g).sum())
    base = R.adam_clip_ref(torch.float64, p, g, m, v, **hp)
    extra = R.adam_clip_ref(torch.float64, p, g, m, v, extra_sumsq=3.0 * own, **hp)
    total = R.adam_clip_ref(torch.float64, p, g, m, v, total_sumsq=4.0 * own, **hp)
    assert float(base[3]) == pytest.approx(own ** 0.5, rel=1e-14) and float(extra[3]) == float(base[3]) == float(total[3])
    # norm^2 + 3 norm^2 = (2 norm)^2: the same clip either way, half the coefficient of the plain call
    assert torch.allclose(extra[1], total[1], rtol=1e-14, atol=0) and not torch.allclose(extra[1], base[1], rtol=1e-6, atol=0)
    half = R.adam_clip_ref(torch.float64, p, 0.5 * g, m, v, **{**hp, "max_norm": 0.0})
    full = R.adam_clip_ref(torch.float64, p, g, m, v, **{**hp, "max_norm": 2.0 * own ** 0.5 + 2e-6})          # coefficient exactly 1
    assert torch.equal(full[1], R.adam_clip_ref(torch.float64, p, g, m, v, **{**hp, "max_norm": 0.0})[1]) and half[1] is not None


def test_splitmix64_published_vectors():
    """the first outputs of Vigna's splitmix64.c for the seeds 0 and 1234567 (the generator's state advances by the golden-ratio constant)"""
    gamma = 0x9E3779B97F4A7C15
    assert [R.splitmix64(0), R.splitmix64(gamma), R.splitmix64(2 * gamma & R.MASK64)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [R.splitmix64(1234567), R.splitmix64(1234567 + gamma)] == [6457827717110365317, 3203168211198807973]


def test_threshold_labels_tell_a_fused_rescale_from_torchs():
    """the MAE mask (|y| > 5e-5 after the rescale, null value 0) and the MAPE mask (|y| >= 1e-4) of the 801 labels around -mean / std, from
    torch's float32 ``y * std + mean`` and from a rescale rounded once: at least 6 labels in total must differ for MAE and at least 1 for
    MAPE (measured: 7 and 1), none for the control scaler (150, 200)"""
    mae_flips = mape_flips = 0
    for std, mean in R.SCALERS:
        y = R.threshold_labels(std, mean)
        assert y.numel() == 801 and y.dtype == torch.float32 and bool((y[1:] != y[:-1]).all())
        two, one = R.torch_rescale(y, std, mean), R.fused_rescale(y, std, mean)
        a = int((R.mae_mask(two, 0.0) != R.mae_mask(one, 0.0)).sum())
        b = int((R.mape_mask(two)[1] != R.mape_mask(one)[1]).sum())
        masked = int((~R.mae_mask(two, 0.0)).sum())
        print(f"scaler ({std}, {mean}): MAE mask flips {a}, MAPE mask flips {b}, labels masked {masked} of {y.numel()}")
        assert 0 < masked < y.numel()          # the labels straddle the threshold
        if (std, mean) == (150.0, 200.0):
            assert a == 0 and b == 0
        else:
            mae_flips += a
            mape_flips += b
    assert mae_flips >= 6 and mape_flips >= 1, (mae_flips, mape_flips)


def _loss_case(seed, B=2, N=7, nan_pred=False, nan_label=False, all_masked=False):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, 12, N, 1, generator=g)
    real = torch.randn(B, 12, N, 1, generator=g)
    real[0, :, 2] = -200.0 / 150.0
    if all_masked:
        real[:] = -200.0 / 150.0
    if nan_pred:
        pred[1, 3, 4] = float("nan")
    if nan_label:
        real[1, 5, 1] = float("nan")
    theta = torch.rand(B, N, N, generator=g).clamp(1e-4, 1 - 1e-4)
    prior = (torch.rand(B, N, N, generator=g) < 0.2).float()
    return pred, real, theta, prior


@pytest.mark.parametrize("kind", ["plain", "nan_pred", "nan_label", "all_masked"])
def test_loss_reference_is_the_oracles_step_loss(kind):
    """loss_ref(float32) against oracle.step_oracle.step_loss and step_amd.step_loss.step_loss on the rescaled float32 tensors: the value,
    and both gradients; a NaN prediction's own gradient is 0 in all of them (the backward of ``where(isnan(loss), 0, loss)``), like the
    recorded reference cases e0 / e11"""
    from step_amd.step_loss import step_loss as package_step_loss
    mean, std = 200.0, 150.0
    pred, real, theta, prior = _loss_case(3, nan_pred=kind == "nan_pred", nan_label=kind == "nan_label", all_masked=kind == "all_masked")
    ref = R.loss_ref(torch.float32, pred, real, theta, prior, 0.7, 0.0, std, mean)
    p = pred.clone().requires_grad_(True)
    t = theta.clone().requires_grad_(True)
    want = O.step_loss(O.rescale(p, mean, std), O.rescale(real, mean, std), t, prior, 0.7, null_val=0.0)
    also = package_step_loss(p * std + mean, real * std + mean, t, prior, 0.7, null_val=0.0)
    assert float(ref["loss"]) == pytest.approx(float(want.detach()), rel=2e-6) and float(also.detach()) == pytest.approx(float(want.detach()), rel=2e-6)
    assert torch.isfinite(ref["loss"]) and torch.isfinite(ref["dpred"]).all()
    gp, gt = torch.autograd.grad(want, [p, t])
    assert torch.isfinite(gp).all()
    assert torch.allclose(ref["dpred"], gp, rtol=1e-5, atol=0) and torch.allclose(ref["dtheta"], gt, rtol=1e-5, atol=1e-12)
    if kind == "nan_pred":
        assert float(ref["dpred"][1, 3, 4]) == 0.0 and float(gp[1, 3, 4]) == 0.0 and bool(ref["mask"][1, 3, 4])
    n = pred.numel()
    assert ref["count"] == {"plain": n - 12, "nan_pred": n - 12, "nan_label": n - 12, "all_masked": 0}[kind]          # a NaN label counts
    if kind == "all_masked":
        assert float(ref["dpred"].abs().max()) == 0.0
    r64 = R.loss_ref(torch.float64, pred, real, theta, prior, 0.7, 0.0, std, mean)
    assert float(r64["loss"]) == pytest.approx(float(ref["loss"]), rel=1e-5) and torch.equal(r64["mask"], ref["mask"])


def test_metrics_reference_in_float64_keeps_the_float32_masks():
    gen = torch.Generator().manual_seed(4)
    y = torch.randn(3, 12, 9, 1, generator=gen) * 50 + 100
    y[0, :, 1] = 0.0
    y[1, :, 2] = 3e-5
    y[2, 0, 0] = float("nan")
    for v, at in ((5e-5, 3), (1e-4, 4)):          # exactly on, and one step either side of, both thresholds
        t = torch.tensor(v, dtype=torch.float32)
        y[2, 1, at], y[2, 2, at], y[2, 3, at] = t, torch.nextafter(t, torch.tensor(1.0)), torch.nextafter(t, torch.tensor(0.0))
    p = y + torch.randn(y.shape, generator=gen) * 10
    p[1, 1, 1] = float("nan")
    m32, m64 = R.masked_metrics_ref(p, y, 0.0), R.masked_metrics_ref(p, y, 0.0, dtype=torch.float64)
    assert m32.dtype == torch.float32 and m64.dtype == torch.float64 and torch.isfinite(m64).all()
    assert torch.allclose(m32.double(), m64, rtol=1e-5, atol=0)
    # against the oracle's masked_mae (the one of the three that the oracle has)
    assert float(m32[0]) == pytest.approx(float(O.masked_mae(p, y, 0.0)), rel=2e-6)
    t = torch.tensor([5e-5])          # float32(5e-5) is "close" to 0 (<=), the next float32 is not
    assert R.mae_mask(torch.cat([t, torch.nextafter(t, torch.tensor([1.0]))]), 0.0).tolist() == [False, True]
