"""Validation and test passes spread over two ranks on one device (tests/eval_spread_worker.py, tests/spread_double.py; gloo, one attempt):
``STEP.evaluate(process_group=...)`` and ``native_runner(..., spread_eval=True)`` against the single-process passes, with and without the
graph learner in time slices, and a rank whose vote fails.  The bound and what was measured for it: the worker's docstring.  Host side:
tests/test_eval_spread_host.py."""
import inspect

import pytest

from tests.two_ranks import run_two_ranks

pytestmark = pytest.mark.gpu


def test_the_switches_are_arguments_of_native_runner_and_evaluate():
    from step_amd import STEP
    from step_amd.evaluate import EvalMetrics, evaluate_pass
    from step_amd.runner import native_runner
    from tests.spread_double import SpreadRunnerDouble
    for name, default in (("eval_noise", "position"), ("native_test", False), ("spread_eval", False)):
        assert inspect.signature(native_runner).parameters[name].default == default
    native_runner(SpreadRunnerDouble, native_data_parallel=True, native_eval=True, native_test=True, eval_noise="window", spread_eval=True)
    assert inspect.signature(STEP.evaluate).parameters["process_group"].default is None
    assert inspect.signature(evaluate_pass).parameters["process_group"].default is None and hasattr(EvalMetrics, "all_reduce")


def test_evaluate_over_a_process_group_equals_the_single_process_pass(tmp_path):
    run_two_ranks("eval_spread_worker.py", "evaluate", tmp_path, timeout=300)


def test_runner_spreads_the_passes_and_a_failed_vote_keeps_them_on_rank_0(tmp_path):
    run_two_ranks("eval_spread_worker.py", "runner", tmp_path, timeout=300)


def test_runner_spreads_the_passes_behind_the_gather_of_the_time_slices(tmp_path):
    run_two_ranks("eval_spread_worker.py", "shard", tmp_path, timeout=300)
