"""``native_runner(..., native_data_parallel=True)`` with two ranks on one device around easytorch's distributed protocol
(tests/dp_double.py, tests/dp_runner_worker.py): the module leaves its DistributedDataParallel wrap, the fused optimizer and the native
iteration act as for one process, the sampler still gets ``set_epoch``, rank 0's checkpoint keeps the reference's format, the replicas
stay bit-identical -- and a replica that does not is found at the start of the next epoch, on every rank."""
import pytest

from tests.two_ranks import run_two_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ("pretrain", "step"))
def test_the_runner_trains_data_parallel_without_the_wrap(kind, tmp_path):
    run_two_ranks("dp_runner_worker.py", kind, tmp_path, timeout=300)
