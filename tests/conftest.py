import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _cpu_threads(workers):
    """intra-op threads per test process.  The oracle passes of the parity tests are 64 x 64-tile networks: on the GPU
    box's 256 host threads torch's default (one OpenMP thread per core) spends its time in barriers - the round-2 suite
    took 1001 s that way, 103 s with 6 workers x 20 threads (gpurun_out/r03_t0.log)."""
    n = os.cpu_count() or 8
    return max(4, min(20, n // max(workers, 1)))


def _workers(config):
    """xdist workers: none unless XV2_TEST_WORKERS asks for them (an explicit -n is left to xdist).  Every worker keeps
    its own HIP context open for the whole run and a multi-rank test adds its rank processes on the same GPU; in one
    process the suite holds the GPU in at most six processes at a time: the test process and at most 5 rank children
    (tests/test_dist_gpu.py sizes its largest worlds to that)."""
    env = os.environ.get("XV2_TEST_WORKERS")
    if env is None or getattr(config.option, "numprocesses", None) is not None:
        return 0
    return max(0, int(env))


@pytest.hookimpl(tryfirst=True)
def pytest_cmdline_main(config):
    """`XV2_TEST_WORKERS=N pytest -m gpu`: spread the parity tests over N xdist workers (each with its own HIP context
    on the one GPU and a bounded OpenMP team for its oracle passes).  xdist's own pytest_cmdline_main runs last and
    turns numprocesses into worker specs.  Without the variable everything runs in one process."""
    if not config.pluginmanager.hasplugin("xdist") or os.environ.get("PYTEST_XDIST_WORKER"):
        return None
    n = _workers(config)
    if n > 0:
        config.option.numprocesses = n
        os.environ.setdefault("OMP_NUM_THREADS", str(_cpu_threads(n)))
    return None


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    if os.environ.get("OMP_NUM_THREADS") is None and (os.cpu_count() or 1) >= 32:
        # single-process runs on a many-core host: same cap (set before torch spins up its thread pool)
        os.environ["OMP_NUM_THREADS"] = str(_cpu_threads(1))
    try:
        import torch
        want = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
        if want > 0 and torch.get_num_threads() > want:
            torch.set_num_threads(want)
    except Exception:
        pass


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
