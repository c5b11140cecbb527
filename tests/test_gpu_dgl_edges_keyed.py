"""``step_dgl_edges_forward_keyed`` called directly (ctypes, outside ``STEP``): the graph learner's Gumbel noise keyed by an int64 per
sample instead of by the sample's position in the batch.

* exactness: the host restatement of the counter layout (tests/edges_keyed_host.py, Philox4x32-10 pinned to known-answer vectors in
  tests/test_eval_spread_host.py) gives ``u [B, N*N, 2]``; the EXISTING ``step_dgl_edges_forward`` run on that ``u`` must equal the keyed
  call bit for bit in theta, adj and the whole of ``saved`` -- everything behind (u0, u1) is one kernel body;
* invariance: a key's row does not depend on the batch it sits in or on its position; equal keys give equal rows;
* statistics of tests/test_gpu_dgl_edges_direct.py::test_device_noise on fixed seeds and keys (checked on the host restatement first:
  tests/test_eval_spread_host.py runs the same function on the float64 oracle's sample);
* N = 65536 is refused before anything is launched.
"""
import ctypes

import pytest
import torch

from tests import direct_ref as D
from tests import edges_keyed_host as K

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (3, 37), (8, 64), (2, 260)]
SEED = (0x1234 << 32) | 0x9ABCDEF1          # both key words of the generator in use


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("B,N", SHAPES)
def test_keyed_equals_existing_path_on_restated_noise(B, N):
    c = D.cached_edge_case(B, N)
    keys = K.keys_of(B)
    keyed = K.run_edges(c, keys=keys, seed=SEED)
    plain = K.run_edges(c, u=K.keyed_uniform(keys, N, SEED), seed=SEED)
    assert bool(torch.isfinite(keyed["saved"]).all()) and bool(torch.isfinite(keyed["adj"]).all())          # every NaN byte was overwritten
    for k in ("theta", "adj", "saved"):
        assert torch.equal(_bits(keyed[k]), _bits(plain[k])), k
    eye = torch.eye(N, dtype=torch.bool)
    assert bool((keyed["adj"][:, eye] == 0).all()) and bool(((keyed["adj"] == 0) | (keyed["adj"] == 1)).all())


@pytest.mark.parametrize("N", [37, 64])
def test_a_keys_row_does_not_depend_on_its_batch(N):
    c = D.cached_edge_case(8, N)
    keys = K.keys_of(8)
    full = K.run_edges(c, keys=keys, seed=SEED)
    k = keys[5]
    alone = K.run_edges(c, keys=[k], seed=SEED)
    assert torch.equal(_bits(alone["adj"][0]), _bits(full["adj"][5])) and torch.equal(_bits(alone["theta"][0]), _bits(full["theta"][5]))
    assert keys[1] == keys[2] and torch.equal(full["adj"][1], full["adj"][2])          # duplicate keys: one draw
    assert not torch.equal(full["adj"][0], full["adj"][1])                              # another key
    assert not torch.equal(K.run_edges(c, keys=[k], seed=SEED + 1)["adj"], alone["adj"])          # another seed
    # a key that differs in its high word only is another stream
    assert not torch.equal(K.run_edges(c, keys=[k + (1 << 32)], seed=SEED)["adj"], alone["adj"])
    # the positional stream under the same seed is another stream (tags 0x5EED / 0x5EEE)
    pos = D.run_edges(c, use_u=False, seed=SEED, backward=False)
    assert not torch.equal(pos["adj"][0], full["adj"][0])


@pytest.mark.parametrize("B,N", K.STAT_SHAPES)
def test_keyed_noise_statistics(B, N):
    c = D.cached_edge_case(B, N)
    keys = K.keys_of(B)
    a = K.run_edges(c, keys=keys, seed=K.STAT_SEEDS[0])
    again = K.run_edges(c, keys=keys, seed=K.STAT_SEEDS[0])
    other = K.run_edges(c, keys=keys, seed=K.STAT_SEEDS[1])
    assert torch.equal(a["adj"], again["adj"]) and torch.equal(a["theta"], again["theta"])
    assert not torch.equal(a["adj"], other["adj"])
    K.check_statistics(a["theta"], a["adj"], other["theta"], other["adj"], keys, tag=f"B={B} N={N}")


def test_too_many_nodes_is_refused_before_a_launch():
    """N = 65536: e = i * N + j no longer fits the one counter word -- STEP_ERR_ARG (1); the pointers are never dereferenced"""
    from step_amd import _lib as L
    from step_amd.step_arch.discrete_graph_learning import fill_dgl_struct
    dev = torch.device("cuda")
    c = D.cached_edge_case(1, 2)
    struct = fill_dgl_struct({k: v.to(dev).contiguous() for k, v in c["ep"].items()}, 0)
    small = torch.zeros(16, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    rc = L.lib().step_dgl_edges_forward_keyed(L.ptr(small), 65536, 1, ctypes.byref(struct), L.ptr(key), 1, D.TEMPERATURE, L.ptr(small),
                                              L.ptr(small), L.ptr(small), L.stream())
    assert rc == 1 and b"65535" in L.lib().step_last_error()
    torch.cuda.synchronize()
    assert bool((small == 0).all())
    rc = L.lib().step_dgl_edges_forward_keyed(L.ptr(small), 2, 1, ctypes.byref(struct), None, 1, D.TEMPERATURE, L.ptr(small),
                                              L.ptr(small), L.ptr(small), L.stream())
    assert rc == 1
