"""torch.optim.Adam's state format for an optimizer whose graph learner is cut in time slices (``FusedAdamClip(gathered_state=True)``),
on CPU tensors and without the library: the column cut and paste shared by the module and the optimizer, a torch state loaded into the
sliced optimizers of two ranks and assembled again, the refusals, the runner's vote (``shard_decision``), and ``gather_state`` itself
between two gloo processes (tests/shard_state_host_worker.py).

The stand-in follows tests/test_optim_state_host.py -- small parameters with padding, a frozen one first, ``fc_w`` last behind the spare
slot -- around a REAL ``DiscreteGraphLearning`` on the CPU, so that ``_shard``, the bounds and ``fc_weight_slice`` are the module's own.
Through the runner, on the device: tests/test_gpu_shard_runner.py."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from step_amd.optim import FusedAdamClip
from step_amd.runner import MIN_SLICE_COLUMNS, native_runner, shard_decision
from step_amd.step_arch.discrete_graph_learning import DiscreteGraphLearning, cut_time_columns, paste_time_columns
from tests.test_abi_and_host import _free_port
from tests.test_optim_state_host import HYPER, HostFused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("b", "a", "c", "d")          # flat order, in front of the spare slot and dgl.fc_w


class ShardHostModel(torch.nn.Module):
    """the surface of ``STEP`` that FusedAdamClip's state conversions read, with a graph learner that can be sliced"""

    def __init__(self, T2, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        for name, shape in (("frozen", (5,)), ("a", (2,)), ("b", (3,)), ("c", (2, 5)), ("d", (4, 4))):
            setattr(self, name, torch.nn.Parameter(torch.randn(*shape, generator=gen), requires_grad=name != "frozen"))
        torch.manual_seed(seed)
        self.discrete_graph_learning = DiscreteGraphLearning("SYNTH", 3, 12, 12, data=np.zeros((T2 + 18, 4, 1), np.float32),
                                                             train_length=T2 + 18, tsformer_tokens=1)
        self.T2 = T2
        self._flat_param = None

    def shard(self, rank, world):
        """what ``enable_native_data_parallel(shard_graph_learner=True)`` and the optimizer's constructor leave behind"""
        self.discrete_graph_learning.shard_time_slices(rank, world)
        return self.flatten()

    def flatten(self):
        self._flat_param = torch.zeros(self._grad_layout()["total"])
        return self

    def _trainable(self):
        dgl = self.discrete_graph_learning
        return [(k, getattr(self, k)) for k in SMALL] + [("dgl.fc_w", dgl.fc.weight if dgl._shard is None else dgl.fc_weight_slice)]

    def _grad_layout(self):
        off, items, order, slot = 0, {}, [], None
        for k, v in self._trainable():
            if k == "dgl.fc_w":
                slot = off
                off += 4
            items[k] = (off, v.numel(), tuple(v.shape))
            order.append(k)
            off += (v.numel() + 3) & ~3
        return {"items": items, "order": order, "total": off, "norm_slot": slot}

    def adam_params(self):
        """the list the replaced Adam was built around BEFORE anyone sliced: no ``fc_weight_slice`` in it"""
        sl = self.discrete_graph_learning._parameters.get("fc_weight_slice")
        return [p for p in self.parameters() if p is not sl]


class SlicedHostFused(HostFused):
    def __init__(self, model, params=None, gathered_state=True, **hyper):
        self.gathered_state = gathered_state
        super().__init__(model, params, **hyper)


def stepped_params(model):
    return [getattr(model, k) for k in SMALL] + [model.discrete_graph_learning.fc.weight]


def adam_after(model, steps, first=0):
    """torch's Adam over ALL parameters of an unsliced ``model``; only the five of the flat buffer ever get a gradient"""
    opt = torch.optim.Adam(model.parameters(), **HYPER)
    adam_steps(opt, model, steps, first)
    return opt


def adam_steps(opt, model, steps, first=0):
    for it in range(first, first + steps):
        gen = torch.Generator().manual_seed(100 + it)
        for p in stepped_params(model):
            p.grad = torch.randn(*p.shape, generator=gen)
        opt.step()


def two_ranks_loaded(T2, sd, source, world=2):
    out = []
    for rank in range(world):
        m = ShardHostModel(T2)
        m.load_state_dict(source.state_dict())
        m.shard(rank, world)
        f = SlicedHostFused(m, params=m.adam_params())
        f.load_state_dict(sd)
        out.append((m, f))
    return out


def assemble(ranks):
    """what ``gather_state`` leaves on rank 0, without a process group: every rank's slice pasted into two full tensors"""
    m0, f0 = ranks[0]
    (at, (T2, _, _)), = f0._sliced.items()
    _, off, p = f0._index[at]
    staged = tuple(torch.full(p.shape, float("nan")) for _ in range(2))
    for m, f in ranks:
        sh = m.discrete_graph_learning._shard
        n = m.discrete_graph_learning.fc_weight_slice.numel()
        for full, buf in zip(staged, (f.exp_avg, f.exp_avg_sq)):
            paste_time_columns(full, T2, sh["a"], sh["b"], buf[off:off + n])
    return {at: staged}


# ---------------------------------------------------------------------------------------------- cut and paste
@pytest.mark.parametrize("T2", (683, 257, 385))
@pytest.mark.parametrize("world", (1, 2, 3))
def test_cut_then_paste_reproduces_the_matrix_and_cuts_tile_it(T2, world):
    rows, ch = 5, 16
    full = torch.randn(rows, ch * T2, generator=torch.Generator().manual_seed(T2 + world))
    bounds = DiscreteGraphLearning.slice_bounds(T2, world)
    assert bounds[0] == 0 and bounds[-1] == T2 and all(b > a for a, b in zip(bounds, bounds[1:]))
    if world > 1 and T2 % world:
        assert len({b - a for a, b in zip(bounds, bounds[1:])}) == 2          # uneven
    back = torch.full_like(full, float("nan"))
    seen = torch.zeros(rows, ch, T2, dtype=torch.int32)
    for a, b in zip(bounds, bounds[1:]):
        piece = cut_time_columns(full, T2, a, b)
        assert piece.shape == (rows, ch * (b - a)) and piece.is_contiguous()
        assert piece.untyped_storage().data_ptr() != full.untyped_storage().data_ptr() or world == 1
        assert torch.equal(piece.view(rows, ch, b - a), full.view(rows, ch, T2)[:, :, a:b])
        seen[:, :, a:b] += 1
        paste_time_columns(back, T2, a, b, piece)
    assert bool((seen == 1).all())          # disjoint, and together the whole
    assert torch.equal(back, full)
    flat_piece = cut_time_columns(full, T2, bounds[0], bounds[1]).reshape(-1)          # a 1-D piece, as a flat buffer hands it over
    again = torch.zeros_like(full)
    paste_time_columns(again, T2, bounds[0], bounds[1], flat_piece)
    assert torch.equal(again.view(rows, ch, T2)[:, :, :bounds[1]], full.view(rows, ch, T2)[:, :, :bounds[1]])


def test_the_module_methods_cut_what_they_always_cut():
    T2 = 257
    m = ShardHostModel(T2).discrete_graph_learning
    w0 = m.fc.weight.detach().clone()
    sh = m.shard_time_slices(1, 2)
    a, b = sh["a"], sh["b"]
    assert (a, b) == (128, 257) and not m.fc.weight.requires_grad
    old = w0.view(100, 16, T2)[:, :, a:b].contiguous().view(100, -1)          # the expression shard_time_slices held before
    assert torch.equal(m.fc_weight_slice.detach(), old) and m.fc_weight_slice.requires_grad
    assert m.fc_weight_slice.untyped_storage().data_ptr() != m.fc.weight.untyped_storage().data_ptr()
    with torch.no_grad():
        m.fc.weight.mul_(3.0)
    m.refresh_fc_weight_slice()
    assert torch.equal(m.fc_weight_slice.detach(), (3.0 * w0).view(100, 16, T2)[:, :, a:b].reshape(100, -1))
    whole = ShardHostModel(T2).discrete_graph_learning          # one slice: the cut is the whole matrix, and still a copy
    whole.shard_time_slices(0, 1)
    assert torch.equal(whole.fc_weight_slice.detach(), whole.fc.weight.detach())
    assert whole.fc_weight_slice.untyped_storage().data_ptr() != whole.fc.weight.untyped_storage().data_ptr()


# ---------------------------------------------------------------------------------------------- torch's format over slices
def test_binding_puts_the_slice_at_fc_weights_position_with_the_full_shape():
    T2 = 683
    m = ShardHostModel(T2).shard(1, 2)
    params = m.adam_params()
    f = SlicedHostFused(m, params=params)
    at = next(i for i, p in enumerate(params) if p is m.discrete_graph_learning.fc.weight)
    assert f._sliced == {at: (T2, 341, 683)}
    name, off, p = f._index[at]
    assert name == "dgl.fc_w" and p is m.discrete_graph_learning.fc.weight and tuple(p.shape) == (100, 16 * T2)
    lay = m._grad_layout()
    assert off == lay["items"]["dgl.fc_w"][0] == lay["norm_slot"] + 4 and lay["items"]["dgl.fc_w"][1] == 100 * 16 * 342
    assert f.flat.numel() == off + 100 * 16 * 342
    assert sorted(v[0] for v in f._index.values()) == ["a", "b", "c", "d", "dgl.fc_w"] and f._label[0] == "frozen"
    # the default list (model.parameters() of the sliced module) also holds fc.weight
    assert SlicedHostFused(m)._sliced is not None
    # an unsliced model ignores the flag
    plain = ShardHostModel(T2).flatten()
    g = SlicedHostFused(plain)
    assert g._sliced is None and g._index is not None
    g.gather_state()          # no slices: nothing to gather, no process group needed
    assert g._staging is None and g.state_dict()["state"] == {}


@pytest.mark.parametrize("T2", (683, 257))
def test_a_torch_state_loads_into_two_ranks_and_comes_back_bit_for_bit(T2):
    source = ShardHostModel(T2)
    adam = adam_after(source, 3)
    sd = adam.state_dict()
    ranks = two_ranks_loaded(T2, sd, source)
    (at, _), = ranks[0][1]._sliced.items()
    for m, f in ranks:
        sh = m.discrete_graph_learning._shard
        assert f.step_count == 3
        _, off, _ = f._index[at]
        n = 100 * 16 * (sh["b"] - sh["a"])
        assert f.exp_avg.numel() == off + n
        for key, buf in (("exp_avg", f.exp_avg), ("exp_avg_sq", f.exp_avg_sq)):
            assert torch.equal(buf[off:off + n].view(100, -1), cut_time_columns(sd["state"][at][key], T2, sh["a"], sh["b"])), key
            gaps = torch.ones(buf.numel(), dtype=torch.bool)
            for o, k, _ in m._grad_layout()["items"].values():
                gaps[o:o + k] = False
            assert int(gaps.sum()) >= 4 and not buf[gaps].any()          # padding and the spare slot stay zero
    m0, f0 = ranks[0]
    f0._staging = assemble(ranks)
    back = f0.state_dict()
    assert back["param_groups"] == sd["param_groups"] and sorted(back["state"]) == sorted(sd["state"])
    for i, st in sd["state"].items():
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert back["state"][i][key].shape == st[key].shape and torch.equal(back["state"][i][key], st[key]), (i, key)
    # ... and a torch Adam over an UNSLICED model loads it and steps like the source
    twin = ShardHostModel(T2)
    twin.load_state_dict(source.state_dict())
    fresh = torch.optim.Adam(twin.parameters())
    fresh.load_state_dict(copy.deepcopy(back))
    adam_steps(adam, source, 1, first=3)
    adam_steps(fresh, twin, 1, first=3)
    for (n, p), q in zip(source.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), n
        assert (q in fresh.state) == (p in adam.state)
        if p in adam.state:
            assert float(fresh.state[q]["step"]) == 4.0
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(fresh.state[q][key], adam.state[p][key]), (n, key)
    # loading its own emitted state keeps the slice, and drops the staging it came from
    m, v = f0.exp_avg.clone(), f0.exp_avg_sq.clone()
    f0.load_state_dict(back)
    assert f0._staging is None and f0.step_count == 3 and torch.equal(f0.exp_avg, m) and torch.equal(f0.exp_avg_sq, v)


def test_gather_state_of_a_single_slice_needs_no_process_group():
    T2 = 257
    source = ShardHostModel(T2)
    sd = adam_after(source, 2).state_dict()
    (m, f), = two_ranks_loaded(T2, sd, source, world=1)
    f.gather_state()
    (at, (mm, vv)), = f._staging.items()
    assert torch.equal(mm, sd["state"][at]["exp_avg"]) and torch.equal(vv, sd["state"][at]["exp_avg_sq"])
    assert mm.untyped_storage().data_ptr() != f.exp_avg.untyped_storage().data_ptr()          # staging, not a view
    out = f.state_dict()["state"]
    assert out[at]["exp_avg"] is mm and out[1]["exp_avg"].untyped_storage().data_ptr() == f.exp_avg.untyped_storage().data_ptr()
    f.release_state()
    with pytest.raises(RuntimeError, match=r"gather_state\(\)"):
        f.state_dict()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_are_by_name():
    T2 = 257
    source = ShardHostModel(T2)
    good = adam_after(source, 3).state_dict()
    (m0, f0), (m1, f1) = two_ranks_loaded(T2, good, source)
    (at, _), = f0._sliced.items()
    before = f1.exp_avg.clone()

    def refused(sd, match):
        with pytest.raises(ValueError, match=match):
            f1.load_state_dict(sd)
        assert f1.step_count == 3 and torch.equal(f1.exp_avg, before)          # nothing was written

    sd = copy.deepcopy(good)
    sd["state"][at]["exp_avg"] = torch.zeros(100, 16 * 129)          # this rank's slice shape is not what torch's format carries
    refused(sd, r"exp_avg of 'dgl.fc_w' .*\(100, 2064\).*\(100, 4112\)")
    sd = copy.deepcopy(good)
    sd["state"][at]["exp_avg_sq"] = torch.zeros(16 * T2, 100)
    refused(sd, "exp_avg_sq of 'dgl.fc_w'")
    sd = copy.deepcopy(good)
    del sd["state"][at]
    refused(sd, "4 of the 5 parameters.*none for 'dgl.fc_w'")
    sd = copy.deepcopy(good)
    del sd["state"][1]
    refused(sd, "4 of the 5 parameters.*none for 'a'")
    sd = copy.deepcopy(good)
    sd["state"][0] = copy.deepcopy(sd["state"][1])
    refused(sd, "entry for 'frozen'.*not in the flat buffer")
    # a step has run (three, loaded) and nobody gathered: neither rank may emit its slice as the whole
    for f in (f0, f1):
        with pytest.raises(RuntimeError, match=r"stepped since the last gather.*gather_state\(\) on ALL ranks"):
            f.state_dict()
    # after a gather rank 0 holds the staging, the other ranks nothing: they refuse too
    f0._staging, f1._staging = assemble([(m0, f0), (m1, f1)]), {}
    assert sorted(f0.state_dict()["state"]) == sorted(good["state"])
    with pytest.raises(RuntimeError, match=r"gather_state\(\) assembled .* on the group's rank 0"):
        f1.state_dict()
    # stale: whatever changes the moments drops the staging
    f0.load_state_dict(good)
    with pytest.raises(RuntimeError, match=r"gather_state\(\)"):
        f0.state_dict()
    # before the first step there is nothing to gather: the empty state, on any rank
    fresh = SlicedHostFused(m1, params=m1.adam_params())
    assert fresh.state_dict()["state"] == {} and fresh.state_dict()["param_groups"][0]["params"] == list(range(len(m1.adam_params())))


def test_without_the_flag_a_sliced_optimizer_keeps_the_flat_per_rank_format():
    T2 = 257
    source = ShardHostModel(T2)
    good = adam_after(source, 2).state_dict()
    m = ShardHostModel(T2).shard(0, 2)
    f = SlicedHostFused(m, params=m.adam_params(), gathered_state=False)
    assert f._index is None and f._sliced is None
    with pytest.raises(ValueError, match="with a sharded graph learner the optimizer state is the flat per-rank format"):
        f.load_state_dict(good)
    n = f.flat.numel()
    mm, vv = torch.rand(n), torch.rand(n)
    f.load_state_dict({"step": 7, "exp_avg": mm, "exp_avg_sq": vv, "param_groups": [dict(HYPER, lr=5e-4)]})
    out = f.state_dict()
    assert sorted(out) == ["exp_avg", "exp_avg_sq", "param_groups", "step"] and out["step"] == 7
    assert out["exp_avg"] is f.exp_avg and torch.equal(f.exp_avg, mm) and torch.equal(f.exp_avg_sq, vv) and "params" not in out["param_groups"][0]
    f.gather_state()          # nothing bound: a no-op
    assert f._staging is None
    # the flat per-rank format still loads with the flag set
    g = SlicedHostFused(m, params=m.adam_params())
    g.load_state_dict(out)
    assert g.step_count == 7 and torch.equal(g.exp_avg, mm) and g.param_groups[0]["lr"] == 5e-4
    assert inspect_default("gathered_state", FusedAdamClip.__init__) is False


def inspect_default(name, f):
    import inspect
    return inspect.signature(f).parameters[name].default


# ---------------------------------------------------------------------------------------------- the runner's vote and its switch
def test_the_vote_is_unsharded_unless_everything_holds():
    assert MIN_SLICE_COLUMNS == 128
    assert shard_decision("bf16", 683, 2, True) is True
    assert shard_decision("f32", 683, 2, True) is False          # f32 mode
    assert shard_decision("bf16", 683, 2, False) is False          # the optimizer stays torch's
    assert shard_decision("bf16", 255, 2, True) is False          # 127 and 128 columns
    assert DiscreteGraphLearning.slice_bounds(255, 2) == [0, 127, 255]
    assert shard_decision("bf16", 256, 2, True) is True          # 128 and 128
    assert shard_decision("bf16", 385, 3, True) is True and shard_decision("bf16", 383, 3, True) is False          # 128,128,129 / 127,128,128
    assert shard_decision("bf16", 13581, 2, True) is True and shard_decision("bf16", 13581, 8, True) is True          # STEP_PEMS04
    assert shard_decision("bf16", 683, 1, True) is False          # a single rank has nothing to share


def test_the_switch_exists_is_off_by_default_and_refuses_accumulation(tmp_path):
    from tests.dp_double import DistributedRunnerDouble
    from tests.resume_double import ResumeRunnerDouble
    from tests.runner_double import RunnerDouble
    assert inspect_default("shard_graph_learner", native_runner) is False
    cfg = {"model": torch.nn.Linear(2, 2), "loss": None, "scaler": (0.0, 1.0), "ckpt_dir": str(tmp_path)}
    runner = native_runner(DistributedRunnerDouble, native_data_parallel=True, shard_graph_learner=True, accumulate=2)(cfg)
    with pytest.raises(ValueError, match="shard_graph_learner=True cannot be combined with accumulate=2"):
        runner.init_training({})
    assert runner.optim is None          # raised before the base class built anything
    assert runner._shard_acting is False
    # a base with on_epoch_end gets the gather in front of it; one with save_model alone, in front of that; one with neither, nothing

    class WithEpochEnd(ResumeRunnerDouble):
        def on_epoch_end(self, epoch):
            return ("ended", epoch)

    a, b, c = native_runner(WithEpochEnd), native_runner(ResumeRunnerDouble), native_runner(RunnerDouble)
    assert "on_epoch_end" in vars(a) and "save_model" not in vars(a)
    assert "save_model" in vars(b) and "on_epoch_end" not in vars(b)
    assert "save_model" not in vars(c) and "on_epoch_end" not in vars(c)
    assert a(cfg).on_epoch_end(3) == ("ended", 3)          # the switch does not act: the base class's call, nothing else


# ---------------------------------------------------------------------------------------------- gather_state between two processes
def test_two_cpu_ranks_gather_the_moments_onto_rank_0(tmp_path):
    """one attempt; a worker that hangs is killed with the other one and the test fails"""
    script = os.path.join(ROOT, "tests", "shard_state_host_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, script, ROOT, str(tmp_path)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and "ok" in o, o[-4000:]
