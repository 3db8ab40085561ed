"""The launch workspace's carve (nsd_launch_workspace_layout), without a GPU:
for every batch size and grid, what the fused kernel, the split schedule
with static tiles and the split schedule with a shared tail keep in the
workspace lies in regions that are disjoint where they are used together,
aligned as the kernels index them, and inside nsd_workspace_bytes(n)."""
import ctypes
import random

import nsd

MAX_GRID = 4096          # NSD_MAX_GRID
BLOCK, WAVES = 256, 4


def _layout(n, blocks, compact):
    L = nsd.lib()
    L.nsd_launch_workspace_layout.restype = ctypes.c_int
    L.nsd_launch_workspace_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_uint64)]
    out = (ctypes.c_uint64 * 20)()
    assert L.nsd_launch_workspace_layout(n, blocks, compact, out) == 0
    return [int(x) for x in out]


def _sizes():
    rnd = random.Random(3)
    ns = {1, 2, 63, 64, 65, 255, 256, 257, (1 << 24) + 1}
    for k in range(9, 25):
        ns |= {(1 << k) - 1, 1 << k, (1 << k) + 1, rnd.randrange(1 << (k - 1), 1 << k)}
    # a wave's share of 15, 16 and 17 tiles (the shared tail's threshold) at a few grids
    for b in (1, 3, 8, 512, 768):
        ns |= {64 * WAVES * b * r + d for r in (15, 16, 17) for d in (0, 17)}
    blocks = [1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 512, 768, 1023, 1024,
              2047, 2048, 4095, 4096]
    return sorted(ns), blocks


def test_rejects_empty_arguments():
    L = nsd.lib()
    L.nsd_launch_workspace_layout.restype = ctypes.c_int
    L.nsd_launch_workspace_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_uint64)]
    out = (ctypes.c_uint64 * 20)()
    assert L.nsd_launch_workspace_layout(0, 1, 1, out) < 0
    assert L.nsd_launch_workspace_layout(1, 0, 1, out) < 0
    assert L.nsd_launch_workspace_layout(1, 1, 1, None) < 0


def test_regions_disjoint_aligned_and_inside():
    ns, grids = _sizes()
    shared = 0
    for n in ns:
        total = int(nsd.lib().nsd_workspace_bytes(n))
        for want_blocks in grids:
            for compact in (0, 1):
                (tot, fp_at, fp_b, gt_at, gt_b, pair_at, pair_b, sl_at, sl_b, sp_at, sp_b, dl_at, dl_b, dp_at,
                 dp_b, fits, cap_s, cap_d, trounds, heads) = _layout(n, want_blocks, compact)
                where = f"n={n} blocks={want_blocks} compact={compact}"
                blocks = min(want_blocks, MAX_GRID, ((n + 63) // 64 + WAVES - 1) // WAVES)
                rounds = -(-n // (blocks * BLOCK))
                assert tot == total, where
                # tile counters and the sample's pair: after everything else, in this order
                assert gt_at % 128 == 0 and pair_at % 8 == 0, where
                assert gt_at + 128 * MAX_GRID <= pair_at and pair_at + pair_b <= total, where
                assert gt_b == (128 * blocks if compact else 0) and pair_b == 16, where
                # the fused kernel's pending lists: u64 slots from the start, below the counters
                assert fp_at == 0 and fp_b % 8 == 0 and fp_b <= gt_at, where
                # the split schedule, both carves: lists of two uint4 a slot, then u64 pending lists
                for l_at, l_b, p_at, p_b, cap in ((sl_at, sl_b, sp_at, sp_b, cap_s), (dl_at, dl_b, dp_at, dp_b, cap_d)):
                    assert l_at == 0 and l_b == 32 * blocks * WAVES * cap, where
                    assert p_at % 256 == 0 and l_b <= p_at and p_b == 8 * blocks * WAVES * cap, where
                assert sp_at + sp_b <= gt_at, where         # the static carve always fits
                assert cap_s == 64 * rounds, where          # a slot for every packet of a wave's share
                assert cap_d == cap_s + cap_s // 5, where   # a fifth more for a wave that takes more
                assert fits == (dp_at + dp_b <= gt_at), where
                # the shared tail: only where its carve fits and the share is 16 tiles or more
                if fits and rounds >= 16:
                    assert trounds == rounds // 2 + ((rounds - rounds // 2) & 1) and rounds - trounds >= 4, where
                    assert (rounds - trounds) % 2 == 0, where   # an even front (a pair per turn of the unrolled loop)
                    shared += 1
                else:
                    assert trounds == 0, where
                assert 1 <= heads <= 256 and (heads == 1 or blocks // heads >= 16), where
                assert heads < 8 or heads % 8 == 0, where
    assert shared > 1000


def test_layout_values_pinned():
    """The values themselves, not only their properties: the 20 words of every
    (n, blocks, compact) of _sizes(), packed little-endian in enumeration
    order, hash to what the launcher computed before the layout moved into
    ws_layout (the kernels' pointer arguments are made of these numbers; a
    change of the carve on purpose updates the digest)."""
    import hashlib
    import struct
    ns, grids = _sizes()
    h = hashlib.sha256()
    for n in ns:
        for want_blocks in grids:
            for compact in (0, 1):
                h.update(struct.pack("<20Q", *_layout(n, want_blocks, compact)))
    assert h.hexdigest() == "ac033e87977b85cd4b2eff09eca903cd462a3b651b177f6eecff0be03053f89b"


def test_shared_carve_fits_the_benchmark_shapes():
    """16M packets on 2 and 3 blocks per CU of 256 CUs: the shared tail's lists
    fit the bytes nsd_workspace_bytes returns (no growth)."""
    for blocks in (512, 768):
        out = _layout(1 << 24, blocks, 1)
        assert out[15] == 1 and out[18] > 0
        assert out[13] + out[14] <= out[3]
