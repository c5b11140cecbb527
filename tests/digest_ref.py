"""numpy restatement of libstep_hip's ``step_replica_digest`` (include/step_hip.h, "replica digest"): the oracle of
tests/test_gpu_replica_digest.py, itself pinned to hand-computed values by tests/test_dp_runner_host.py."""
import numpy as np


def mix64(z):
    """the finaliser of splitmix64 on a uint64 array (products wrap mod 2^64)"""
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest(values):
    """float32 array [n] -> (sum mod 2^64, xor) of mix64((i << 32) | bits of values[i]) as Python ints"""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        m = mix64((np.arange(bits.size, dtype=np.uint64) << np.uint64(32)) | bits)
        return int(np.add.reduce(m, dtype=np.uint64)), int(np.bitwise_xor.reduce(m))


def as_int64_pair(words):
    """the two uint64 words as torch exposes them (int64 bit patterns)"""
    return [w - (1 << 64) if w >= (1 << 63) else w for w in words]
