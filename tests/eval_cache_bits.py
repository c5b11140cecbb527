"""The bit layout of the evaluation cache's stored kNN prior (include/step_hip.h, step_frozen_cache_store), defined in numpy:
bit b of word w of row i <-> adj[i][32 w + b] != 0, bits of columns >= N are 0.  The GPU tests compare the kernels against this."""
import numpy as np


def pack_prior_bits(adj):
    """adj [..., N, N] (any numeric dtype) -> uint32 [..., N, ceil(N / 32)]"""
    a = np.asarray(adj) != 0
    N = a.shape[-1]
    W = (N + 31) // 32
    b = np.packbits(a, axis=-1, bitorder="little")                     # [..., ceil(N / 8)] bytes, column 0 in bit 0 of byte 0
    pad = np.zeros(b.shape[:-1] + (4 * W - b.shape[-1],), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([b, pad], axis=-1)).view("<u4")


def unpack_prior_bits(words, N):
    """uint32 [..., N, W] -> float32 [..., N, N] of exactly 0.0 / 1.0"""
    b = np.ascontiguousarray(np.asarray(words).astype("<u4")).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :N].astype(np.float32)
