"""Gradient accumulation under ``enable_native_data_parallel`` with two ranks on one device (tests/dp_grad_accum_worker.py), STEP and the
pre-training TSFormer, k = 2: the collectives are issued in the group's second backward only, the reduced gradient is the mean over the
ranks of each rank's sum, and the replicas stay bit-identical through two optimizer steps -- over ``torch.distributed`` and over RCCL's C
API (tests/fake_rccl stands in for librccl, which refuses two ranks on one device)."""
import pytest

from tests.two_ranks import fake_rccl, run_two_ranks

pytestmark = pytest.mark.gpu


def test_accumulating_data_parallel_training_with_two_ranks_on_one_device():
    run_two_ranks("dp_grad_accum_worker.py", timeout=300, env={"STEP_RCCL_LIB": fake_rccl()})
