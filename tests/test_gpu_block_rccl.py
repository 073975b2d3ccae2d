"""The block halo exchange through RCCL on one GPU, over a 1-rank communicator (see tests/rccl_loopback_block.py): once in the
single-stream ordering (the loopback operator is small: the default) and once in the two-stream ordering under plain events
(SAENA_SINGLE_STREAM_NNZ=0; the block path has no polling ordering to fall into)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORDERINGS = {"single-stream": {"SAENA_SINGLE_STREAM_NNZ": str(10 ** 9)}, "two-streams-events": {"SAENA_SINGLE_STREAM_NNZ": "0"}}


@pytest.mark.parametrize("ordering", list(ORDERINGS))
def test_rccl_loopback_block(ordering):
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "tests.rccl_loopback_block", "--torch"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **ORDERINGS[ordering])
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "RCCL_LOOPBACK_BLOCK_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
