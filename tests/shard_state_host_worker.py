"""Worker of tests/test_shard_state_host.py: one process per rank, gloo group, everything on the CPU (no kernel is launched).

``FusedAdamClip.gather_state`` between two ranks with uneven slices (T2 = 257: 128 and 129 columns): every rank loads the same torch
state, marks its moments with its rank so that a slice pasted from the wrong rank shows, and gathers.  Rank 0's staging is the
concatenation of the ranks' slices; rank 1 holds nothing and refuses ``state_dict()``; ``gather_fc_weight`` next to it leaves the same
matrix on both ranks."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
from step_amd.step_arch.discrete_graph_learning import cut_time_columns                                  # noqa: E402
from tests.test_shard_state_host import ShardHostModel, SlicedHostFused, adam_after                     # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
T2 = 257
source = ShardHostModel(T2)          # seeded: the same on both ranks
sd = adam_after(source, 2).state_dict()
m = ShardHostModel(T2)
m.load_state_dict(source.state_dict())
m.shard(rank, world)
dgl = m.discrete_graph_learning
sh = dgl._shard
assert (sh["a"], sh["b"]) == ((0, 128), (128, 257))[rank]
f = SlicedHostFused(m, params=m.adam_params())
f.load_state_dict(sd)
(at, _), = f._sliced.items()
_, off, p = f._index[at]
n = dgl.fc_weight_slice.numel()
assert f.exp_avg.numel() == off + n
f.exp_avg[off:off + n] += 10.0 * (rank + 1)          # this rank's mark on its slices
f.exp_avg_sq[off:off + n] += 100.0 * (rank + 1)
f.gather_state()
if rank == 0:
    (k, (mm, vv)), = f._staging.items()
    assert k == at and mm.shape == vv.shape == (100, 16 * T2)
    for r, (a, b) in enumerate(((0, 128), (128, 257))):
        assert torch.equal(cut_time_columns(mm, T2, a, b), cut_time_columns(sd["state"][at]["exp_avg"], T2, a, b) + 10.0 * (r + 1)), r
        assert torch.equal(cut_time_columns(vv, T2, a, b), cut_time_columns(sd["state"][at]["exp_avg_sq"], T2, a, b) + 100.0 * (r + 1)), r
    out = f.state_dict()
    assert out["state"][at]["exp_avg"] is mm and all(float(st["step"]) == 2.0 for st in out["state"].values())
    torch.optim.Adam(source.parameters()).load_state_dict(out)          # torch's Adam over the unsliced model takes it
else:
    assert f._staging == {}
    try:
        f.state_dict()
        raise AssertionError("rank 1 has no complete state to give")
    except RuntimeError as ex:
        assert "rank 0" in str(ex) and "gather_state()" in str(ex)
f.release_state()
assert f._staging is None
# a second gather, and the module's own gather next to it (the order of the runner's on_epoch_end)
with torch.no_grad():
    dgl.fc_weight_slice.add_(float(rank + 1))
w0 = source.discrete_graph_learning.fc.weight.detach()
dgl.gather_fc_weight()
f.gather_state()
want = w0.clone().view(100, 16, T2)
want[:, :, :128] += 1.0
want[:, :, 128:] += 2.0
assert torch.equal(dgl.fc.weight.detach(), want.view(100, -1))
assert (f._staging != {}) == (rank == 0)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", flush=True)
