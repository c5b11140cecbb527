"""FusedAdamClip's optimizer state in torch.optim.Adam's format, on CPU tensors and without the library: the two conversions of
step_amd/optim.py (flat moment buffers <-> ``{"state", "param_groups"}``) against a live ``torch.optim.Adam`` over plain parameters, the
errors for states the fused pass cannot hold, the flat format of earlier checkpoints, and the runner's hand-over of a resumed optimizer
and scheduler (step_amd/runner.py, ``hand_over_training_state``).

The layout is hand-made after ``STEP._grad_layout()``: parameters of 3, 2, 10, 16 and 33 floats (every one starts at a multiple of
four, so all but one are followed by padding), a four-float spare slot in front of ``fc_w``, flat order different from the order of
``params``, and one frozen parameter FIRST in ``params`` (positions are not flat ranks).  On the device: tests/test_gpu_resume.py."""
import copy

import pytest
import torch

from step_amd.optim import FusedAdamClip, adam_group, flat_items, index_flat_items, moments_to_state, state_to_moments
from step_amd.runner import hand_over_training_state

HYPER = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-7, weight_decay=1e-5)
FLAT_ORDER = ("b", "a", "c", "d", "fc_w")          # fc_w last, behind the spare slot, as in STEP._trainable()


class HostModel(torch.nn.Module):
    """the surface of ``STEP`` that FusedAdamClip's state conversions read"""

    def __init__(self, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        for name, shape in (("frozen", (5,)), ("a", (2,)), ("b", (3,)), ("c", (2, 5)), ("fc_w", (3, 11)), ("d", (4, 4))):
            setattr(self, name, torch.nn.Parameter(torch.randn(*shape, generator=gen), requires_grad=name != "frozen"))
        self._flat_param = torch.zeros(self._grad_layout()["total"])

    def _trainable(self):
        return [(k, getattr(self, k)) for k in FLAT_ORDER]

    def _grad_layout(self):
        off, items, order = 0, {}, []
        for k, v in self._trainable():
            if k == "fc_w":
                off += 4
            items[k] = (off, v.numel(), tuple(v.shape))
            order.append(k)
            off += (v.numel() + 3) & ~3
        return {"items": items, "order": order, "total": off}


class HostFused(FusedAdamClip):
    """FusedAdamClip without its device buffers: the methods under test only touch the moments, the step count and the groups"""

    def __init__(self, model, params=None, **hyper):
        self.model, self.flat = model, model._flat_param
        torch.optim.Optimizer.__init__(self, [self.flat], dict(hyper or HYPER))
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.max_norm, self.step_count, self.dyn = None, 0, None
        self._bind_params(params)


def gradients(model, it):
    gen = torch.Generator().manual_seed(100 + it)
    return {k: torch.randn(*p.shape, generator=gen) for k, p in model._trainable()}


def adam_after(model, steps, **hyper):
    """torch's Adam over ALL parameters of ``model`` (the frozen one never gets a gradient, so never a state entry)"""
    opt = torch.optim.Adam(model.parameters(), **(hyper or HYPER))
    for it in range(steps):
        for k, g in gradients(model, it).items():
            getattr(model, k).grad = g
        opt.step()
    return opt


def bound(model, params=None):
    params = list(model.parameters()) if params is None else params
    return index_flat_items(flat_items(model), params, {id(p): n for n, p in model.named_parameters()})


def in_gaps(model, buf):
    """the floats of a flat buffer that belong to no parameter: padding and the spare slot"""
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    for off, n, _ in model._grad_layout()["items"].values():
        keep[off:off + n] = False
    return buf[keep]


def test_the_layout_has_padding_a_spare_slot_and_a_frozen_first_parameter():
    model = HostModel()
    lay = model._grad_layout()
    assert sorted(n for _, n, _ in lay["items"].values()) == [2, 3, 10, 16, 33] and lay["total"] == 76
    assert lay["items"]["fc_w"][0] == lay["items"]["d"][0] + 16 + 4
    params = list(model.parameters())
    assert params[0] is model.frozen
    index, label = bound(model)
    assert {i: v[0] for i, v in index.items()} == {1: "a", 2: "b", 3: "c", 4: "fc_w", 5: "d"} and label[0] == "frozen"
    assert [index[i][1] for i in (2, 1, 3, 5, 4)] == [0, 4, 8, 20, 40]          # flat order is not the order of params


def test_torch_state_round_trips_through_the_flat_buffers():
    model = HostModel()
    sd = adam_after(model, 3).state_dict()
    index, label = bound(model)
    m, v = torch.full((76,), float("nan")), torch.full((76,), float("nan"))
    assert state_to_moments(index, label, sd, m, v) == 3
    assert in_gaps(model, m).numel() == 76 - 64 and (in_gaps(model, m) == 0).all() and (in_gaps(model, v) == 0).all()
    back = {"state": moments_to_state(index, m, v, 3), "param_groups": [adam_group(HYPER, 6)]}
    assert back["param_groups"] == sd["param_groups"]
    assert sorted(back["state"]) == sorted(sd["state"]) == [1, 2, 3, 4, 5]
    for i, st in sd["state"].items():
        got = back["state"][i]
        assert sorted(got) == sorted(st)
        assert got["step"].dtype == torch.float32 and got["step"].dim() == 0 and got["step"].device.type == "cpu"
        assert torch.equal(got["step"], st["step"])
        for key in ("exp_avg", "exp_avg_sq"):
            assert got[key].shape == st[key].shape and torch.equal(got[key], st[key])
            assert got[key].untyped_storage().data_ptr() == (m if key == "exp_avg" else v).untyped_storage().data_ptr()      # a view, no copy


def test_emitted_state_loads_into_a_fresh_adam_which_steps_like_the_source():
    model = HostModel()
    source = adam_after(model, 3)
    fused = HostFused(model)
    fused.load_state_dict(source.state_dict())
    assert fused.step_count == 3
    twin = HostModel()
    twin.load_state_dict(model.state_dict())
    fresh = torch.optim.Adam(twin.parameters())          # torch's own defaults: everything comes from the loaded groups
    emitted = fused.state_dict()
    assert sorted(emitted) == ["param_groups", "state"]
    fresh.load_state_dict(copy.deepcopy(emitted))
    for i, (p, q) in enumerate(zip(model.parameters(), twin.parameters())):
        assert (q in fresh.state) == (p in source.state) == (i != 0)
        if i:
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(fresh.state[q][key], source.state[p][key]), (i, key)
    want = torch.optim.Adam(model.parameters(), **HYPER).state_dict()["param_groups"]
    got = fresh.state_dict()["param_groups"]
    assert got == want and list(got[0]) == list(want[0]) and "decoupled_weight_decay" in got[0]
    for k, g in gradients(model, 3).items():
        getattr(model, k).grad = g
        getattr(twin, k).grad = g.clone()
    source.step()
    fresh.step()
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), n
        if n != "frozen":
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(fresh.state[q][key], source.state[p][key]), (n, key)
            assert float(fresh.state[q]["step"]) == 4.0


def test_no_entries_before_the_first_step_and_an_empty_state_is_a_fresh_optimizer():
    model = HostModel()
    fused = HostFused(model)
    sd = fused.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == list(range(6))
    torch.optim.Adam(model.parameters()).load_state_dict(sd)
    fused.load_state_dict(adam_after(model, 2).state_dict())
    assert fused.step_count == 2 and float(fused.exp_avg.abs().max()) > 0
    fused.load_state_dict(torch.optim.Adam(model.parameters(), **HYPER).state_dict())
    assert fused.step_count == 0 and not fused.exp_avg.any() and not fused.exp_avg_sq.any()


def test_loading_its_own_live_state_keeps_the_moments():
    model = HostModel()
    fused = HostFused(model)
    fused.load_state_dict(adam_after(model, 3).state_dict())
    m, v = fused.exp_avg.clone(), fused.exp_avg_sq.clone()
    fused.load_state_dict(fused.state_dict())          # the entries are views of the buffers they are copied into
    assert fused.step_count == 3 and torch.equal(fused.exp_avg, m) and torch.equal(fused.exp_avg_sq, v)


@pytest.mark.parametrize("kind", ("int", "float", "tensor"))
def test_step_is_accepted_as_int_float_and_tensor(kind):
    model = HostModel()
    sd = adam_after(model, 3).state_dict()
    for st in sd["state"].values():
        st["step"] = {"int": 3, "float": 3.0, "tensor": torch.tensor(3.0)}[kind]
    fused = HostFused(model)
    fused.load_state_dict(sd)
    assert fused.step_count == 3 and type(fused.step_count) is int


def test_group_options_are_taken_over_and_initial_lr_is_emitted():
    model = HostModel()
    adam = adam_after(model, 1)
    sched = torch.optim.lr_scheduler.MultiStepLR(adam, milestones=[1], gamma=0.5)
    sched.step()
    fused = HostFused(model, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=1.0)
    fused.load_state_dict(adam.state_dict())
    g = fused.param_groups[0]
    assert (g["lr"], g["initial_lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, 2e-3, (0.9, 0.95), 1e-7, 1e-5)
    assert g["params"][0] is fused.flat
    assert fused.state_dict()["param_groups"] == adam.state_dict()["param_groups"]


def test_a_state_the_fused_pass_cannot_hold_is_refused_by_name():
    model = HostModel()
    good = adam_after(model, 3).state_dict()
    before = HostFused(model)
    before.load_state_dict(good)

    def refused(sd, match):
        fused = HostFused(model)
        fused.load_state_dict(good)
        with pytest.raises(ValueError, match=match):
            fused.load_state_dict(sd)
        assert fused.step_count == 3 and torch.equal(fused.exp_avg, before.exp_avg)          # nothing was written

    sd = copy.deepcopy(good)
    sd["state"][3]["exp_avg"] = torch.zeros(5, 2)
    refused(sd, r"exp_avg of 'c' .*\(5, 2\).*\(2, 5\)")
    sd = copy.deepcopy(good)
    sd["state"][4]["exp_avg_sq"] = torch.zeros(33)
    refused(sd, "exp_avg_sq of 'fc_w'")
    sd = copy.deepcopy(good)
    sd["state"][0] = copy.deepcopy(sd["state"][1])
    refused(sd, "entry for 'frozen'.*not in the flat buffer")
    sd = copy.deepcopy(good)
    sd["state"][5]["step"] = torch.tensor(4.0)
    refused(sd, "'d' at step 4")
    sd = copy.deepcopy(good)
    del sd["state"][2]
    refused(sd, "4 of the 5 parameters.*none for 'b'")
    sd = copy.deepcopy(good)
    sd["param_groups"][0]["params"] = list(range(5))
    refused(sd, "saved around 5 parameters.*given 6")


def test_every_flat_parameter_must_be_among_params():
    model = HostModel()
    with pytest.raises(ValueError, match="lacks 1 parameter.*'d'"):
        HostFused(model, params=[p for n, p in model.named_parameters() if n != "d"])
    trainable = [p for p in model.parameters() if p.requires_grad]          # what the easytorch stand-in of the tests hands to Adam
    fused = HostFused(model, params=trainable)
    adam = torch.optim.Adam(trainable, **HYPER)
    for it in range(2):
        for k, g in gradients(model, it).items():
            getattr(model, k).grad = g
        adam.step()
    fused.load_state_dict(adam.state_dict())
    sd = fused.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3, 4] and sd["param_groups"][0]["params"] == list(range(5))
    assert torch.equal(sd["state"][3]["exp_avg"], adam.state[model.fc_w]["exp_avg"])


def test_the_flat_format_of_earlier_checkpoints_still_loads():
    model = HostModel()
    fused = HostFused(model)
    m, v = torch.rand(76), torch.rand(76)
    fused.load_state_dict({"step": 7, "exp_avg": m, "exp_avg_sq": v, "param_groups": [dict(HYPER, lr=5e-4, initial_lr=2e-3)]})
    assert fused.step_count == 7 and torch.equal(fused.exp_avg, m) and torch.equal(fused.exp_avg_sq, v)
    assert fused.param_groups[0]["lr"] == 5e-4 and fused.param_groups[0]["initial_lr"] == 2e-3


def test_scheduler_hand_over_continues_the_uninterrupted_schedule():
    """MultiStepLR(milestones=[1, 3], gamma=0.5) from 2e-3: 2e-3, 1e-3, 1e-3, 5e-4, 5e-4.  The run is interrupted after epoch 2; what the
    resume protocol leaves is a fresh scheduler with ``last_epoch = 2`` on the checkpoint's groups (lr 1e-3, initial_lr 2e-3)."""
    param = {"milestones": [1, 3], "gamma": 0.5}
    model = HostModel()
    straight = torch.optim.Adam(model.parameters(), **HYPER)
    s = torch.optim.lr_scheduler.MultiStepLR(straight, **param)
    rates = []
    for _ in range(4):
        s.step()
        rates.append(straight.param_groups[0]["lr"])
    assert rates == pytest.approx([1e-3, 1e-3, 5e-4, 5e-4], rel=1e-12)

    saved = adam_after(model, 2)
    ss = torch.optim.lr_scheduler.MultiStepLR(saved, **param)
    ss.step()
    ss.step()
    checkpoint = copy.deepcopy(saved.state_dict())
    assert checkpoint["param_groups"][0]["lr"] == pytest.approx(1e-3) and checkpoint["param_groups"][0]["initial_lr"] == 2e-3
    old = torch.optim.Adam(model.parameters(), **HYPER)
    old_sched = torch.optim.lr_scheduler.MultiStepLR(old, **param)
    old.load_state_dict(checkpoint)
    old_sched.last_epoch = 2
    left = copy.deepcopy(old_sched.state_dict())

    fused = HostFused(model, lr=old.param_groups[0]["lr"])          # the decayed rate, as the runner builds it
    new = hand_over_training_state(old, old_sched, fused, param)
    assert type(new) is torch.optim.lr_scheduler.MultiStepLR and new.optimizer is fused
    assert new.state_dict() == left and new.last_epoch == 2 and new.base_lrs == [2e-3]
    assert fused.param_groups[0]["lr"] == checkpoint["param_groups"][0]["lr"] and fused.param_groups[0]["initial_lr"] == 2e-3
    assert fused.step_count == 2 and torch.equal(fused.state_dict()["state"][4]["exp_avg"], checkpoint["state"][4]["exp_avg"])
    assert len(old.state) == 0          # the replaced Adam's moments are released
    got = []
    for _ in range(2):
        new.step()
        got.append(fused.param_groups[0]["lr"])
    assert got == pytest.approx(rates[2:], rel=1e-12) and got == pytest.approx([5e-4, 5e-4], rel=1e-12)
    assert hand_over_training_state(torch.optim.Adam(model.parameters(), **HYPER), None, HostFused(model)) is None
