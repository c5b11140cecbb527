"""libstep_hip ``step_replica_digest`` on the device against its numpy restatement (tests/digest_ref.py, pinned to hand-computed values in
tests/test_dp_runner_host.py).  Both reductions are exact, so every comparison is for equality.  The sizes cross every path of the
kernel: fewer elements than a vector, whole vectors with and without a scalar tail, one wave, more than one wave, more than one
workgroup (a workgroup takes 4096 elements), and bases that are not 16-byte aligned (a scalar head of three and of two elements)."""
import functools

import numpy as np
import pytest
import torch

from tests.digest_ref import as_int64_pair, digest

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 65543)
LARGEST = max(SIZES) + 2


@functools.lru_cache(maxsize=None)
def host_values():
    """float32 [LARGEST] with -0.0, +0.0, a NaN, an inf and denormals among the first elements (every size but n = 1 sees several)"""
    rng = np.random.default_rng(11)
    v = rng.standard_normal(LARGEST).astype(np.float32)
    special = np.array([-0.0, 0.0, np.nan, np.inf, 1e-42, -3e-45, -np.inf], dtype=np.float32)
    v[:special.size] = special
    v[-4:] = np.array([1e-40, np.nan, -0.0, 7.0], dtype=np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def device_values():
    return torch.from_numpy(host_values().copy()).cuda()


def device_digest(t):
    from step_amd.comm import replica_digest
    out = replica_digest(t)
    assert out.dtype == torch.int64 and out.shape == (2,) and out.is_cuda
    return out.cpu().tolist()


@pytest.mark.parametrize("offset", (0, 1, 2))
@pytest.mark.parametrize("n", SIZES)
def test_digest_equals_the_reference(n, offset):
    flat = device_values()[offset:offset + n]
    assert flat.data_ptr() % 16 == 4 * offset          # (the cached buffer starts 16-byte aligned)
    want = as_int64_pair(digest(host_values()[offset:offset + n]))
    got = device_digest(flat)
    assert got == want
    assert device_digest(flat) == got                   # two calls give equal words


def test_one_flipped_low_bit_changes_both_words():
    n = 1025
    base = host_values()[:n]
    want = device_digest(device_values()[:n])
    for at in (0, n - 1):
        bits = base.view(np.uint32).copy()
        bits[at] ^= 1
        got = device_digest(torch.from_numpy(bits.view(np.float32)).cuda())
        assert got == as_int64_pair(digest(bits.view(np.float32)))
        assert got[0] != want[0] and got[1] != want[1], at


def test_a_swap_of_two_unequal_elements_shows():
    n = 257
    v = host_values()[:n].copy()
    assert v[10] != v[200]
    before = device_digest(torch.from_numpy(v).cuda())
    v[10], v[200] = v[200], v[10]
    after = device_digest(torch.from_numpy(v).cuda())
    assert after == as_int64_pair(digest(v)) and after != before


def test_the_output_is_overwritten_and_bad_arguments_are_refused():
    import ctypes
    from step_amd import _lib
    flat = device_values()[:4100]
    out = torch.full((2,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    _lib.call("step_replica_digest", _lib.ptr(flat), flat.numel(), _lib.ptr(out), _lib.stream())
    assert out.cpu().tolist() == as_int64_pair(digest(host_values()[:4100]))
    lib = _lib.lib()
    assert lib.step_replica_digest(_lib.ptr(flat), 1 << 32, _lib.ptr(out), _lib.stream()) == 1          # n < 2^32 is a precondition
    assert lib.step_replica_digest(_lib.ptr(flat), 0, _lib.ptr(out), _lib.stream()) == 1
    assert lib.step_replica_digest(None, 4, _lib.ptr(out), _lib.stream()) == 1
    assert lib.step_replica_digest(ctypes.c_void_p(flat.data_ptr() + 2), 4, _lib.ptr(out), _lib.stream()) == 1
    with pytest.raises(ValueError):
        from step_amd.comm import replica_digest
        replica_digest(flat.double())
