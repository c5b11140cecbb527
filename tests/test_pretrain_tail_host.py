"""Host side of the pre-training tail (``TSFormer.pretrain_tail``, ``DevicePretrainingDataset``, ``native_runner(...,
native_pretrain=True)``): the fixture tests/golden/pretrain_tail_cases.npz is what the ORACLE's masked_mae / rescale (pinned to the
reference by tests/test_oracle_golden.py) and the restated metrics of tests/test_train_tail_host.py give on the masked tokens, the
recording tool reproduces the stored file where the reference is at hand, the dataset reads pickles written like the reference's, the
runner keeps the base class's path where the native tail cannot run, and the library's work-buffer size needs no device.
Device side: tests/test_gpu_pretrain_tail.py."""
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import step_oracle as O
from oracle.reference_loader import reference_root
from tests.test_abi_and_host import _DummyBase
from tests.test_train_tail_host import restated_metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pretrain_tail_cases.npz")
CASES = ["a", "b", "c", "d", "e", "e_un"]


def masked_tokens(z, c, r):
    """(reconstruction, label) of the masked tokens of case c, [S, Pm, 12] each: rows Pu + j of r, patches mk[j] of the series"""
    S, P, _ = r.shape
    Pu, mk = int(z[f"{c}.Pu"]), torch.from_numpy(z[f"{c}.mk"]).long()
    return r[:, Pu:, :], torch.from_numpy(z[f"{c}.series"]).view(S, P, 12)[:, mk, :]


def test_fixture_equals_the_oracle_on_the_masked_tokens():
    """same f32 operations on the same CPU: 1e-6 leaves room for the order of a sum only"""
    z = np.load(FIXTURE)
    assert sorted(z["cases"].tolist()) == CASES
    assert os.path.getsize(FIXTURE) < 1 << 20
    shapes = {c: (z[f"{c}.r"].shape, int(z[f"{c}.Pu"]), z[f"{c}.mk"].tolist()) for c in CASES}
    assert shapes["a"] == ((3, 4, 12), 1, [3, 0, 2])
    assert shapes["b"][:2] == ((10, 14, 12), 4) and shapes["b"][2] == sorted(shapes["b"][2])
    assert shapes["c"][:2] == ((74, 28, 12), 7) and shapes["c"][2] == sorted(shapes["c"][2])
    for c in CASES:
        mean, std = float(z[f"{c}.shift"]), float(z[f"{c}.scale"])
        assert z[f"{c}.series"].shape == (z[f"{c}.r"].shape[0], z[f"{c}.r"].shape[1] * 12)
        assert int(z[f"{c}.B"]) * int(z[f"{c}.N"]) == z[f"{c}.r"].shape[0] and z[f"{c}.mk"].dtype == np.int32
        r = torch.from_numpy(z[f"{c}.r"]).clone().requires_grad_(True)
        recon, label = masked_tokens(z, c, r)
        p, y = O.rescale(recon, mean, std), O.rescale(label, mean, std)
        loss = O.masked_mae(p, y, 0.0)
        dr, = torch.autograd.grad(loss, [r])
        assert float(loss.detach()) == pytest.approx(float(z[f"{c}.loss"]), rel=1e-6)
        np.testing.assert_allclose(restated_metrics(p.detach(), y, 0.0).numpy(), z[f"{c}.metrics"], rtol=1e-6, atol=1e-7)
        want = z[f"{c}.dr"]
        nan_at = np.isnan(z[f"{c}.r"])
        assert np.isfinite(want[~nan_at]).all() and int(nan_at.sum()) == (1 if c in ("e", "e_un") else 0)
        np.testing.assert_allclose(dr.numpy()[~nan_at], want[~nan_at], rtol=1e-6, atol=1e-12)
        assert (want[:, :int(z[f"{c}.Pu"])][~nan_at[:, :int(z[f"{c}.Pu"])]] == 0).all()          # the unmasked rows carry no gradient
    # d: nothing counts; e_un: a NaN outside the masked rows changes nothing; e: the NaN is a counted term that adds 0
    assert float(z["d.loss"]) == 0.0 and z["d.metrics"].tolist() == [0.0, 0.0, 0.0] and (z["d.dr"] == 0).all()
    assert z["e_un.loss"] == z["b.loss"] and np.array_equal(z["e_un.metrics"], z["b.metrics"])
    assert np.array_equal(z["e_un.dr"], z["b.dr"])
    assert 0 < float(z["e.loss"]) < float(z["b.loss"])
    where = np.argwhere(np.isnan(z["e.r"]))[0]
    assert where[1] >= int(z["e.Pu"]) and np.argwhere(np.isnan(z["e_un.r"]))[0][1] < int(z["e_un.Pu"])


@pytest.mark.skipif(reference_root() is None, reason="needs the reference sources")
def test_recording_tool_reproduces_the_stored_fixture():
    spec = importlib.util.spec_from_file_location("make_pretrain_tail_golden", os.path.join(ROOT, "tools", "make_pretrain_tail_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got, z = tool.compute(), np.load(FIXTURE)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        a, b = np.asarray(got[key]), z[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if key.split(".")[-1] in ("loss", "metrics", "dr"):          # results: f32 sums on another CPU may be ordered differently
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-12, err_msg=key)
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


def _write_files(tmp_path, index):
    series = np.random.default_rng(0).normal(size=(300, 5, 3)).astype(np.float32)
    with open(tmp_path / "data.pkl", "wb") as f:
        pickle.dump({"processed_data": series}, f)
    with open(tmp_path / "index.pkl", "wb") as f:
        pickle.dump(index, f)
    return str(tmp_path / "data.pkl"), str(tmp_path / "index.pkl")


def test_device_pretraining_dataset_reads_the_reference_files(tmp_path):
    """modelled on test_device_forecasting_dataset_reads_the_reference_files: the reference's three constructor arguments
    (basicts/data/dataset.py), a history of L rows and a future of 12"""
    from step_amd.runner import DevicePretrainingDataset
    L = 48
    idx = {"train": [(t - L, t, t + 12) for t in (48, 50, 200)], "valid": [(52, 100, 112)], "test": [(52, 100, 112)]}
    data, index = _write_files(tmp_path, idx)
    ds = DevicePretrainingDataset(data, index, "train")
    assert len(ds) == 3 and [int(ds[i]) for i in range(3)] == [48, 50, 200] and ds[0].dtype == torch.int64
    assert (ds.history_len, ds.future_len) == (L, 12) and ds.index_only
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=3)))
    assert batch.tolist() == [48, 50, 200] and batch.dtype == torch.int64
    # through worker processes, as the reference's configs ask for (NUM_WORKERS = 2, PIN_MEMORY = True: TSFormer_PEMS04.py:88-89); the
    # device copies of the series never travel to a worker
    ds._loaders[("cuda", 0)] = object()
    assert pickle.loads(pickle.dumps(ds))._loaders == {}
    del ds._loaders[("cuda", 0)]
    assert [b.tolist() for b in torch.utils.data.DataLoader(ds, batch_size=2, num_workers=2)] == [[48, 50], [200]]
    assert len(DevicePretrainingDataset(data, index, "valid")) == 1
    with pytest.raises(FileNotFoundError):
        DevicePretrainingDataset(str(tmp_path / "nope.pkl"), index, "train")
    with pytest.raises(AssertionError):
        DevicePretrainingDataset(data, index, "all")
    with pytest.raises(TypeError):          # the sibling's fourth argument is not part of the reference's constructor
        DevicePretrainingDataset(data, index, "train", 96)


@pytest.mark.parametrize("bad", [[(0, 48, 60), (2, 51, 63)],            # a history of 49 rows
                                 [(0, 48, 60), (2, 50, 61)],            # a future of 11
                                 [(0, 48, 60), (2, 50, 62, 74)],        # not a triple
                                 [(0, 48, 60), (2, 50)],
                                 [(48, 48, 60)],                        # no history at all
                                 []])
def test_device_pretraining_dataset_refuses_a_ragged_index(tmp_path, bad):
    from step_amd.runner import DevicePretrainingDataset
    data, index = _write_files(tmp_path, {"train": bad, "valid": [(0, 48, 60)], "test": [(0, 48, 60)]})
    with pytest.raises(ValueError):
        DevicePretrainingDataset(data, index, "train")
    assert len(DevicePretrainingDataset(data, index, "valid")) == 1


def test_native_pretrain_on_cpu_tensors_takes_the_base_path():
    """modelled on test_native_tail_on_cpu_tensors_takes_the_base_path: no TSFormer on a GPU, so ``native_pretrain=True`` changes nothing"""
    from step_amd.runner import native_runner
    ds = torch.utils.data.TensorDataset(torch.arange(12.0).view(6, 2), torch.arange(12.0).view(6, 2) * 0.5)
    plain = list(torch.utils.data.DataLoader(ds, batch_size=2))
    R = native_runner(_DummyBase, native_pretrain=True)
    r, base = R({}), _DummyBase({})
    assert r._pretrain_module() is None and r._pretrain_scaler(plain[0]) is None
    losses = [(float(r.train_iters(1, it, d)), float(base.train_iters(1, it, d))) for it, d in enumerate(plain)]
    assert all(a == b for a, b in losses)
    r.print_epoch_meters("train")
    base.print_epoch_meters("train")
    assert r.printed == base.printed and not r._pending
    r.init_training({})
    assert isinstance(r.optim, torch.optim.SGD)


def test_a_cpu_tsformer_is_left_alone_by_native_pretrain():
    from step_amd import TSFormer
    from step_amd.runner import native_runner
    r = native_runner(_DummyBase, native_pretrain=True)({})
    r.model = TSFormer(12, 1, 96, 4, 4, 0.1, 4, 0.75, 4, 1, mode="pre-train")
    assert r._pretrain_module() is None
    r.init_training({})
    assert isinstance(r.optim, torch.optim.SGD) and r.model._flat_param is None


def test_work_buffer_size_needs_no_device():
    from step_amd import _lib
    n = _lib.lib().step_pretrain_tail_work_doubles()
    assert isinstance(n, int) and n >= 12 and n == _lib.lib().step_train_tail_work_doubles()          # the scheme of step_train_tail


def test_bad_arguments_are_refused_on_the_host():
    from step_amd import TSFormer
    m = TSFormer(12, 1, 96, 4, 4, 0.1, 4, 0.75, 4, 1, mode="pre-train")
    x = torch.zeros(2, 48, 3, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # CPU tensors: there is no fall-back path
        m.pretrain_tail(x, 0.0, rescale=(200.0, 150.0))
    for nv in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            m.pretrain_tail(x, nv)
    with pytest.raises(ValueError):
        m.pretrain_tail(x[0])
    m.mode = "forecasting"
    with pytest.raises(ValueError, match="pre-train"):
        m.pretrain_tail(x)
