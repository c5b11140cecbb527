"""Launcher of the two-rank GPU tests (test infrastructure): two worker processes, a gloo group over a free local port, both on cuda:0.
One attempt: every worker gets ``communicate(timeout=...)``; on a timeout both are killed and the test fails with what they printed."""
import os
import subprocess
import sys

from tests.test_abi_and_host import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_rccl():
    """tests/fake_rccl built (the shared-memory stand-in for librccl that lets two ranks share one device) -> its path"""
    from tests.test_gpu_comm_two_ranks import build_fake
    return build_fake()


def run_two_ranks(script, *args, timeout=300, env=None):
    """-> the two outputs; asserts that both workers exit 0 after printing "ok" """
    world = 2
    base = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    base.update(env or {})
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", script), ROOT, *[str(a) for a in args]], env=dict(base, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs, timed_out = [], False
    try:
        for p in procs:
            try:
                outs.append(p.communicate(timeout=timeout)[0].decode())
            except subprocess.TimeoutExpired:
                timed_out = True
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if timed_out:
        outs = [p.communicate()[0].decode() for p in procs]
        raise AssertionError("a worker did not finish in {} s; both were killed\n".format(timeout) + "\n".join(o[-3000:] for o in outs))
    print("\n".join(o[-2500:] for o in outs))
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and "ok" in o, o[-4000:]
    return outs
