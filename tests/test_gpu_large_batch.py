"""Every *_dev entry point past 2^32 bytes and at the largest batch dcmt_create admits (65535 frames): code whose correctness
depends on size -- 64-bit frame offsets, flat 32-bit pixel indices, the segment loops of the three segmented entry points, grids
with the frame in y or z, the per-batch scratch tables and the sizes the wrappers pass on -- runs here on a device, at the three
geometries of tests/large_batch_cases.py (A: 65535 x 96 x 176, B: 2512 x 352 x 1216, C: 65535 x 128 x 260), which also holds how
a batch is made from a handful of frames and how the whole output is compared on the device.  One case per entry point and
variant, so that a failure names it; a wrap stays inside the allocations, so it shows as frames that hold the sentinel or another
frame's result, not as a fault.

Memory: each case states what it allocates (the context's two planes, its other scratch, inputs and outputs), asserts that this is
under 40 GB, and skips only where the device has less than that plus a quarter free.  Contexts are created per case; the fixture
below gives everything back to the device behind every case, so that a context's allocations never compete with torch's cache.
A case that leaves the device in an error state ends the session: nothing more is started on a device that has faulted."""
import gc

import pytest

import large_batch_cases as LB

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def release_device_memory():
    yield
    import torch
    gc.collect()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, nothing more is started on it: {e}", returncode=3)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(LB.cases()))
def test_entry_point(name):
    LB.cases()[name].run()
