"""References of the training step's update half (step_amd/csrc/optim.hip: gradient-norm clip + Adam, step_loss and its two
gradients, the three training meters, the replay state's hash) with no device and no library: torch on the CPU in a requested dtype.

Shared by tests/test_optim_ref_host.py (which pins these to torch.optim.Adam / clip_grad_norm_, to oracle.step_oracle.step_loss and
step_amd.step_loss.step_loss, and to published splitmix64 vectors), tests/test_gpu_optim_direct.py, tests/test_gpu_step.py and
tests/test_gpu_graphed_step.py.

One convention runs through the loss and the meters: every DISCRETE decision (the null-value mask, MAPE's small-label replacement) is
taken on torch's float32 values -- the rescale ``y * std + mean`` rounded twice, as the reference's runner computes it -- whatever dtype
the arithmetic after it runs in.  A float64 reference that took its own masks would count a label one float32 step from the threshold
differently from the program it is the reference of."""
import numpy as np
import torch

MASK64 = (1 << 64) - 1
# The two numbers of the tolerance rule (tests/direct_ref.py: Compare) for this family; measured ratios (Adam <= 2.65, loss <= 6.67) and
# why LOSS_M is not 32: docstring of tests/test_gpu_optim_direct.py.  Adam has no atomics: floor 0.  The loss and the meters sum in f64 (atomics that commute up to f64
# rounding) and round the final value to float32 once: floor 2^-24 relative, on the scalar values only.
ADAM_M, LOSS_M = 16.0, 16.0
ADAM_FLOOR, LOSS_FLOOR = 0.0, 2.0 ** -24
SCALERS = [(19.5, 54.4), (100.0, 300.0), (156.5, 207.2), (9.6, 62.6), (7.0, 33.0), (150.0, 200.0)]          # (std, mean); the last: control


# ----------------------------------------------------------------------------------------- clip + Adam
def adam_clip_ref(dtype, p, g, m, v, *, lr, betas, eps, wd, step, max_norm, extra_sumsq=None, total_sumsq=None):
    """``clip_grad_norm_(max_norm)`` followed by one ``torch.optim.Adam`` step (L2 weight decay added to the clipped gradient, bias-corrected
    moments, eps added after the square root) on flat tensors, in ``dtype``.  -> (p', m', v', norm); nothing is modified in place.
    ``norm``: the L2 norm of ``g`` alone.  The clip coefficient is ``min(1, max_norm / (total + 1e-6))`` (``max_norm`` = 0: no clip) with
    total^2 = norm^2 + ``extra_sumsq`` (the squares of gradient elements held elsewhere), or = ``total_sumsq`` when that is given.
    Operation for operation this is torch's ``_single_tensor_adam`` (lerp_, mul_ + addcmul_, sqrt / div / add_, addcdiv_ with the bias
    corrections as Python floats), so the float32 instance equals a float32 torch run bit for bit (tests/test_optim_ref_host.py)."""
    b1, b2 = betas
    p, g, m, v = (t.detach().to(dtype).clone() for t in (p, g, m, v))
    norm = torch.linalg.vector_norm(g)
    if total_sumsq is not None:
        total = torch.as_tensor(total_sumsq, dtype=dtype).sqrt()
    elif extra_sumsq is not None:
        total = (norm * norm + torch.as_tensor(extra_sumsq, dtype=dtype)).sqrt()
    else:
        total = norm
    if max_norm:
        g = g * torch.clamp(max_norm / (total + 1e-6), max=1.0)
    if wd:
        g = g.add(p, alpha=wd)
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))
    return p, m, v, norm


def abi_float(x):
    """a hyperparameter as the C ABI hands it to the device: include/step_hip.h takes lr, the betas, eps, weight_decay, max_norm, the
    scaler's std and mean and the loss coefficient as ``float``.  The device's problem is Adam with THESE values -- beta2 = float32(0.999)
    = 0.99900001287..., whose 1 - beta2 is 1.29e-5 (relative) below 1e-3 -- and its references are given the same ones.
    (torch.optim.Adam on the CPU keeps the Python doubles; against it the native optimizer's second moment is 1.29e-5 of each step's
    contribution low, 6e-6 of the update: figures in tests/test_gpu_optim_direct.py.)"""
    return tuple(abi_float(v) for v in x) if isinstance(x, (tuple, list)) else float(np.float32(x))


def adam_case(n, seed, gscale=1.0):
    """seeded flat inputs of length n: p ~ 0.1 randn, gradients of three steps (gscale * randn), and m, v after two earlier reference
    steps (float32) on the first two of them, so that neither moment starts at zero.  -> p, g, m, v (float32), the gradient of step 3"""
    gen = torch.Generator().manual_seed(seed * 1000003 + n)
    p = 0.1 * torch.randn(n, generator=gen)
    m, v = torch.zeros(n), torch.zeros(n)
    for t in (1, 2):
        g = gscale * torch.randn(n, generator=gen)
        p, m, v, _ = adam_clip_ref(torch.float32, p, g, m, v, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0, step=t, max_norm=0.0)
    return p, gscale * torch.randn(n, generator=gen), m, v


# ----------------------------------------------------------------------------------------- step_dyn_advance
def splitmix64(x):
    """one step of the splitmix64 hash on a 64-bit integer (Steele, Lea, Flood 2014; Vigna's splitmix64.c): the generator's output for the
    state x, which dyn_advance_kernel stores as the next seed offset"""
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


# ----------------------------------------------------------------------------------------- rescale and thresholds
def torch_rescale(y, std, mean):
    """the runner's ``y * std + mean`` on a float32 tensor: two roundings"""
    assert y.dtype == torch.float32
    return y * std + mean


def fused_rescale(y, std, mean):
    """float32(float64(y) * float64(std) + float64(mean)) with std and mean as the float32 values a kernel is handed: what a device that
    contracts the rescale into one fused multiply-add computes (one rounding).  Only used to show that inputs tell the two apart."""
    assert y.dtype == torch.float32
    s, b = float(np.float32(std)), float(np.float32(mean))
    return (y.double() * s + b).float()


def threshold_labels(std, mean, span=400):
    """the 2 * span + 1 float32 values within +-span steps of float32(-mean / std): normalised labels that rescale to within a few
    float32 steps of 0, on both sides of the 5e-5 (MAE mask) and 1e-4 (MAPE) thresholds for the scalers used here"""
    c = np.float32(-mean / std)
    bits = np.array([c], dtype=np.float32).view(np.int32)[0] + np.arange(-span, span + 1, dtype=np.int32)
    return torch.from_numpy(bits.astype(np.int32).view(np.float32).copy())


def mae_mask(y32, null_val):
    """mae.py:17-21 with a finite null value: ~isclose(y, null, atol = 5e-5, rtol = 0) on float32 labels; a NaN label is not close"""
    assert y32.dtype == torch.float32
    return ~torch.isclose(y32, torch.full_like(y32, null_val), atol=5e-5, rtol=0.0)


def mape_mask(y32):
    """mape.py:20-35: labels below 1e-4 become 0, then the mask against the null value 0.  -> (y0, mask)"""
    assert y32.dtype == torch.float32
    y0 = torch.where(torch.abs(y32) < 1e-4, torch.zeros_like(y32), y32)
    return y0, mae_mask(y0, 0.0)


# ----------------------------------------------------------------------------------------- loss
def loss_ref(dtype, pred, real, theta, prior, coef, null_val=0.0, std=1.0, mean=0.0):
    """step_loss (step/step_loss/step_loss.py:5-16 + basicts/metrics/mae.py:5-28) of ``pred * std + mean`` / ``real * std + mean`` with
    arithmetic in ``dtype`` and the mask from the float32 rescale; pred / real: float32 tensors of one shape (normalised values), theta /
    prior of one shape.  -> {"loss", "dpred" (w.r.t. the NORMALISED prediction), "dtheta", "mask" (bool), "count"}.
    With dtype = float32 this is oracle.step_oracle.step_loss / step_amd.step_loss.step_loss on the rescaled tensors
    (tests/test_optim_ref_host.py); like them it gives a NaN prediction's term the value 0 and the gradient 0."""
    assert pred.dtype == torch.float32 and real.dtype == torch.float32
    mask = mae_mask(torch_rescale(real, std, mean), null_val)
    count = int(mask.sum())
    p = pred.detach().to(dtype).requires_grad_(True)
    t = theta.detach().to(dtype).requires_grad_(True)
    s, b = float(np.float32(std)), float(np.float32(mean))          # the scalars are float32 on the device and in torch's float32 run
    ad = ((p * s + b) - (real.to(dtype) * s + b)).abs()
    ad = torch.where(torch.isnan(ad), torch.zeros_like(ad), ad)          # nan_to_num of the product: the element still counts
    mae = (ad * mask.to(dtype)).sum() / count if count else ad.sum() * 0.0
    # nn.BCELoss, as the reference calls it: the logs clamped at -100, and a backward with the denominator max(t (1 - t), 1e-12)
    bce = torch.nn.functional.binary_cross_entropy(t.reshape(-1), prior.to(dtype).reshape(-1))
    loss = mae + bce * coef
    dp, dt = torch.autograd.grad(loss, [p, t], allow_unused=True)
    dp = torch.zeros_like(p) if dp is None else torch.where(torch.isnan(dp), torch.zeros_like(dp), dp)
    dt = torch.zeros_like(t) if dt is None else dt
    return {"loss": loss.detach(), "dpred": dp, "dtheta": dt, "mask": mask, "count": count}


# ----------------------------------------------------------------------------------------- the three training meters
def masked_metrics_ref(p, y, null, dtype=None):
    """masked_mae, masked_rmse, masked_mape of basicts/metrics/{mae,rmse,mape}.py, restated line by line for a finite null value
    (MAPE's own null value is 0).  -> tensor [3].  dtype: the arithmetic's (default: the inputs'); the masks and MAPE's small-label
    replacement are always those of the float32 labels."""
    dtype = dtype or p.dtype
    y32 = y.float()

    def weights(mask):
        m = mask.to(dtype)
        m = m / m.mean()
        return torch.where(torch.isnan(m), torch.zeros_like(m), m)
    m = weights(mae_mask(y32, null))
    pd, yd = p.to(dtype), y.to(dtype)
    mae = torch.nan_to_num(torch.abs(pd - yd) * m, nan=0.0).mean()
    mse = torch.nan_to_num((pd - yd) ** 2 * m, nan=0.0).mean()
    y0_32, mask0 = mape_mask(y32)
    y0 = torch.where(y0_32 == 0, torch.zeros_like(yd), yd)
    m0 = weights(mask0)
    ape = torch.abs(torch.abs(pd - y0) / y0) * m0
    mape = torch.where(torch.isnan(ape), torch.zeros_like(ape), ape).mean()
    return torch.stack([mae, torch.sqrt(mse), mape])
