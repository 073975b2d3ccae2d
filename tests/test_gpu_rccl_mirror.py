"""The exchanged apply under each of its orderings, on the mirror world (tests/rccl_mirror.py, tests/mirror_world.py): one fresh child
process per ordering over a 1-rank communicator, one at a time.  Each child holds every case to the twin's bits, to the forms'
contract and to the oracle, and asserts through sgpu_debug_exchange_mode that its ordering really ran; this module holds the digests
of every output equal across the orderings -- only the synchronisation differs between them, and the single stream has none to get
wrong.

A child that ends by a signal, at its time limit or with a HIP error in its output fails its test, and the parameters after it fail
without starting a child: nothing more is started on a card after a fault."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_gpu_rccl import SYNC_MODES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT = 600

# id -> (torch first, ordering of SYNC_MODES, what sgpu_debug_exchange_mode must report)
WORKERS = {
    "torch-runtime-kernel-flags": (True, "kernel-flags", "kernel-flags"),
    "torch-runtime-value-ops": (True, "stream-value-ops", "value-ops"),
    "torch-runtime-events": (True, "events", "events"),
    "torch-runtime-long-kernel-events": (True, "events-for-long-kernels", "events"),
    "torch-runtime-single-stream": (True, "single-stream", "one-stream"),
    "system-rocm-kernel-flags": (False, "kernel-flags", "kernel-flags"),
}
HIP_ERRORS = ("HIP error", "hipError", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")
_results = {}
_abnormal = []


def worker(key):
    """the child's JSON lines by case; runs it once"""
    if key in _results:
        return _results[key]
    assert not _abnormal, f"not started: an earlier worker ended abnormally ({_abnormal[0]})"
    torch_first, ordering, expect = WORKERS[key]
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), sys.executable, "-m", "tests.rccl_mirror", "--expect", expect] + (["--torch"] if torch_first else [])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **SYNC_MODES[ordering])
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    tail = out.stdout[-1500:] + out.stderr[-3000:]
    if out.returncode < 0 or out.returncode in (124, 137) or out.returncode >= 128 or any(e in out.stdout or e in out.stderr for e in HIP_ERRORS):
        _abnormal.append(f"{key}: exit status {out.returncode}")
        pytest.fail(f"{key} ended abnormally (exit status {out.returncode}): " + tail)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("RCCL_MIRROR_OK"), tail
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    _results[key] = dict(cases={d["case"]: d for d in lines if "case" in d}, served=[d for d in lines if "served" in d][0]["served"], seconds=lines[-1]["seconds"])
    return _results[key]


@pytest.mark.parametrize("key", list(WORKERS))
def test_rccl_mirror(key):
    r = worker(key)
    print(f"{key}: {r['seconds']} s; " + ", ".join(f"{c} {d['seconds']} {'/'.join(d['modes'])}" for c, d in r["cases"].items()))
    if key == list(WORKERS)[0]:
        print("forms by operator: " + "; ".join(f"{f}: {' '.join(ops)}" for f, ops in r["served"].items()))
    from tests import mirror_world as mw
    from tests.test_gpu_forms import FORMS
    assert list(r["cases"]) == [c.name for c in mw.catalogue()] + ["hierarchy/coarsest-direct", "hierarchy/coarsest-CG"]
    assert set(r["served"]) >= {f.key for f in FORMS}
    expect = WORKERS[key][2]
    seen = {m for d in r["cases"].values() for m in d["modes"]}
    assert expect in seen and seen <= {expect, "one-stream", "none"} | ({"kernel-flags"} if expect == "one-stream" else set()), seen
    assert "one-stream" in r["cases"]["dense%5"]["modes"]


def test_every_ordering_gives_the_same_bits():
    """digests of every output of every case -- chains, the fp32 wire, the block twin and the hierarchies included -- are equal
    across the workers, and so are the forms each operator was served by"""
    keys = list(WORKERS)
    base = worker(keys[0])
    for k in keys[1:]:
        r = worker(k)
        assert r["served"] == base["served"], k
        for case, d in base["cases"].items():
            other = r["cases"][case]["digests"]
            assert set(other) == set(d["digests"]), (k, case)
            differ = sorted(n for n in d["digests"] if other[n] != d["digests"][n])
            assert not differ, f"{case}: {k} and {keys[0]} differ in {differ[:8]}"
