import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _usable_cpus():
    """CPUs this process may really use: the affinity mask capped by a cgroup CPU quota (the GPU boxes show 256 cores behind a
    16-CPU quota: torch's default of one thread per visible core makes the oracle's CPU passes several times slower there)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


# The fp32 CPU results in tests/golden/ were computed with this many torch threads.  How a CPU sum is split among threads changes its
# last bits, and a whole training step carries them past the fixtures' bars (at 16 or 32 threads the full-width and step fixtures fail):
# the tests that recompute those results use this count whatever the host has (golden_cpu_threads).
GOLDEN_CPU_THREADS = 8


@pytest.fixture
def golden_cpu_threads():
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_CPU_THREADS)
    yield
    torch.set_num_threads(n)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    import torch
    torch.set_num_threads(min(32, _usable_cpus()))


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)
