"""``TSFormer.enable_native_data_parallel`` with two ranks on one device (tests/dp_pretrain_worker.py): the state broadcast, the mean of the
flat gradient inside backward over ``torch.distributed`` and over RCCL's C API (tests/fake_rccl stands in for librccl, which refuses two
ranks on one device), replicas that stay bit-identical through FusedAdamClip, and ``replicas_identical`` telling when they do not."""
import pytest

from tests.two_ranks import fake_rccl, run_two_ranks

pytestmark = pytest.mark.gpu


def test_data_parallel_pretraining_with_two_ranks_on_one_device():
    run_two_ranks("dp_pretrain_worker.py", timeout=300, env={"STEP_RCCL_LIB": fake_rccl()})
