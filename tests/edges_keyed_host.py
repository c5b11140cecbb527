"""Host restatement of the window-keyed Gumbel noise of ``step_dgl_edges_forward_keyed`` (TEST INFRASTRUCTURE), and a ctypes driver of
the entry point.

Counter layout (include/step_hip.h): sample b, edge e = i * N + j draw Philox4x32-10 at
    c = (e, low 32 bits of key[b], high 32 bits of key[b], 0x5EEE),  k = (low, high 32 bits of the seed)
and u0 / u1 are words 0 / 1 through ``(x >> 8) * 2^-24``.  The positional stream of ``step_dgl_edges_forward`` (u = NULL) has
    c = (low 32 bits of e, high 32 bits of e, b, 0x5EED).
The generator itself is the restatement of tests/enc_dropout_host.py, pinned here to the known-answer vectors published with Random123
(``kat_vectors``: the philox4x32 10-round lines).
"""
import ctypes

import numpy as np
import torch

from tests.enc_dropout_host import M32, philox4x32

TAG_POSITION, TAG_WINDOW = 0x5EED, 0x5EEE

# (counter, key, expected output) of Philox4x32-10: Random123's kat_vectors
KNOWN_ANSWERS = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def window_counters(N, key):
    """uint32 [N*N, 4] counters of one sample under the window tag"""
    e = np.arange(N * N, dtype=np.uint64)
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    c = np.empty((N * N, 4), dtype=np.uint32)
    c[:, 0] = e.astype(np.uint32)
    c[:, 1], c[:, 2], c[:, 3] = k & M32, k >> 32, TAG_WINDOW
    return c


def position_counters(N, b):
    """uint32 [N*N, 4] counters of sample b under the positional tag"""
    e = np.arange(N * N, dtype=np.uint64)
    c = np.empty((N * N, 4), dtype=np.uint32)
    c[:, 0], c[:, 1] = (e & np.uint64(M32)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32)
    c[:, 2], c[:, 3] = b, TAG_POSITION
    return c


def unit(words):
    """u32_to_unit of csrc/common.h: exact in float32"""
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keyed_uniform(keys, N, seed):
    """-> float32 tensor [B, N*N, 2]: the (u0, u1) the keyed kernel draws for the samples with these keys"""
    seed = int(seed)
    out = np.empty((len(keys), N * N, 2), dtype=np.float32)
    for b, key in enumerate(keys):
        r = philox4x32(window_counters(N, key), seed & M32, (seed >> 32) & M32)
        out[b, :, 0], out[b, :, 1] = unit(r[:, 0]), unit(r[:, 1])
    return torch.from_numpy(out)


def run_edges(case, keys=None, u=None, seed=1):
    """``step_dgl_edges_forward_keyed`` on ``keys`` (int64 [B] on the device), or ``step_dgl_edges_forward`` on the explicit noise
    ``u``; theta_out inside ``saved`` as step.py passes it, every buffer pre-filled with NaN bytes.  B is the number of keys / rows of
    u (the case supplies the parameters and the global feature).  -> host copies of theta, adj and the whole of saved."""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    from tests.direct_ref import TEMPERATURE, _nan_floats
    dev = torch.device("cuda")
    N = case["N"]
    B = len(keys) if keys is not None else u.shape[0]
    lib = L.lib()
    ep = {k: v.to(dev).contiguous() for k, v in case["ep"].items()}
    struct = fill_dgl_struct(ep, 0)
    g = case["g"].to(dev).contiguous()
    saved = _nan_floats(lib.step_dgl_edges_saved_floats(B, N), dev)
    to = int(lib.step_dgl_edges_theta_offset(N))
    theta = saved[to:to + B * N * N].view(B, N, N)
    adj = _nan_floats(B * N * N, dev).view(B, N, N)
    if keys is not None:
        kd = torch.tensor([int(k) for k in keys], dtype=torch.int64, device=dev)
        L.call("step_dgl_edges_forward_keyed", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(kd), seed, TEMPERATURE, L.ptr(saved),
               L.ptr(theta), L.ptr(adj), L.stream())
    else:
        ud = u.to(dev).contiguous()
        L.call("step_dgl_edges_forward", L.ptr(g), N, B, ctypes.byref(struct), L.ptr(ud), seed, TEMPERATURE, L.ptr(saved), L.ptr(theta),
               L.ptr(adj), L.stream())
    torch.cuda.synchronize()
    return {"theta": theta.cpu(), "adj": adj.cpu(), "saved": saved.cpu()}


KEYS = {1: [0], 2: [(1 << 32) + 5, 0], 3: [0, 288, 288], 8: [0, 288, 288, (1 << 32) + 5, 289, 1 << 40, 13599, 3394]}


def keys_of(B):
    """the keys of the direct test's shapes: between them 0, a duplicate inside one batch and values >= 2^32, the rest ordinary
    forecast origins"""
    return list(KEYS[B])


def _corr(x, y):
    x, y = x.double().flatten(), y.double().flatten()
    return float((x * y).mean() / (x.pow(2).mean().sqrt() * y.pow(2).mean().sqrt()))


def check_statistics(theta, adj, other_theta, other_adj, keys, tag=""):
    """the statistics of tests/test_gpu_dgl_edges_direct.py::test_device_noise for a keyed sample: P(adj = 1) = theta (Gumbel-max) --
    in ten equally filled bins of theta, sum(adj) within 5 sigma of sum(theta) -- and residuals adj - theta uncorrelated (|r| <=
    6 / sqrt(n)) between samples of different keys and between two seeds (``other_*``: the same keys under another seed).  Samples
    with the same key are one draw: only the first of them enters"""
    B, N = adj.shape[0], adj.shape[1]
    first = [b for b in range(B) if keys[b] not in keys[:b]]
    off = ~torch.eye(N, dtype=torch.bool)
    th, ad = theta[first][:, off].double(), adj[first][:, off].double()
    order = th.flatten().argsort()
    for q, idx in enumerate(order.chunk(10)):
        t, s = th.flatten()[idx], ad.flatten()[idx]
        sigma = float((t * (1 - t)).sum().sqrt())
        z = float(s.sum() - t.sum()) / sigma
        print(f"keyed noise {tag} bin {q}: theta in [{float(t.min()):.3f}, {float(t.max()):.3f}] n={idx.numel()} z={z:+.2f}")
        assert abs(z) <= 5, (q, z)
    n = N * (N - 1)
    res = ad - th
    res_other = other_adj[first][:, off].double() - other_theta[first][:, off].double()
    for a in range(len(first)):
        for b in range(a + 1, len(first)):
            r = _corr(res[a], res[b])
            assert abs(r) <= 6 / n ** 0.5, ("keys", first[a], first[b], r)
        r = _corr(res[a], res_other[a])
        assert abs(r) <= 6 / n ** 0.5, ("seed", first[a], r)


STAT_SHAPES = [(8, 64), (2, 260)]
STAT_SEEDS = (1234, 1235)
