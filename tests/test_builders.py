"""Host-side preconditions of the GPU tests' batch builders, checked from the
CPU oracle alone: what a construction argument assumes of its batch must hold
before the batch is worth a GPU run."""
import pytest

import nsd_testlib as T
import test_device_parity as DP


@pytest.mark.parametrize("mode", [T.PRINT_NORM, T.PRINT_LESS])
def test_ring_eviction_batch_preconditions(mode):
    """_evict_batch (test_ring_eviction_by_construction): every slow packet
    needs seven 128-byte windows, every full tile defers 4..16 packets, the
    slow kinds sit at lanes 0 and 63, slow10 needs a side word, slow14 an
    entry, the leaf kinds are host-rendered and only slow14_leaf records its
    leaf's end."""
    frames, desc, kinds = DP._evict_batch()
    DP._evict_preconditions(frames, desc, kinds, mode)
