// nsd_kernels.hip - CDNA4 (gfx950) kernels for the netsniff-ng dissector chain.
//
// One lane walks one packet (nsd_walk.h).  Layout in HBM:
//   frames  : one byte buffer, frames at arbitrary offsets
//   desc    : u64 per packet (bits 0..39 offset, 40..63 caplen)
//   rec     : 16-byte chain record per packet (nsd_rec), one dwordx4 store per
//             lane -> 1 KiB contiguous per wave
//   ext     : overflow records for deep chains, slots by wave-aggregated atomic
//   counters: u64[64] per-ops / flag counts
//
// Header windows are staged through LDS in "aligned coordinates": a frame at
// byte offset `off` is read from A = off & ~15 in whole 16-byte chunks (every
// load a global_load_dwordx4, whatever the frame's alignment; AF_PACKET rings
// put the MAC header at 2 mod 16), and frame byte o sits at window position
// o + m, m = off & 15.  Window bytes at frame offsets >= caplen are zeroed.
// Each lane's fast-walk window is one LDS row of 20 dwords: 16-byte aligned
// rows take one ds_write_b128 per chunk, and 32 lanes reading the same
// header offset meet at most 2-way in a bank (an odd 17-dword stride was
// conflict-free but needed 4 ds_write_b32 per chunk: 1.3 % slower on C2).
//
// The fast walk finishes every packet whose chain resolves inside its first
// 64 bytes, with the next tile's chunks and the tile after next's descriptors
// in flight while the current tile is walked from LDS only.  The tile's
// other packets go to the wave's walkers, the general walk (walkers):
// per-lane windows staged at each walker's cursor, idle walkers refilled,
// ext spill; ICMPv4 payload checksums longer than a window are summed by the
// block at the end.
//
// One launch per batch, in one of two schedules (the launcher picks, see
// "the schedule" in nsd_launch.hip): fused (dissect_all: a tile's walkers right after its fast
// walk) or split (dissect_fast: the fast walk of every tile first, deferred
// packets listed per wave, then each wave walks its own list).
//
// This file is the one translation unit that compiles the kernels; their code
// is in the headers it includes, and the launcher reaches them through the
// tables at its end.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "nsd_internal.h"
#include "nsd_launch.h"
#include "nsd_walk.h"
// the device code, in the order it builds on itself: staging and record
// stores, the fused kernel, the split kernel (whose tail runs the fused
// kernel's walker pool: nsd_fast.h includes nsd_fused.h)
#include "nsd_stage.h"
#include "nsd_fused.h"
#include "nsd_fast.h"

// ---- the kernels, for the launcher (nsd_launch.hip) -----------------------------
namespace nsd {

kfn fused_kernel(bool compact, int mi, bool ring)
{
	static const kfn kernels[2][3] = {
		{ dissect_all<PRINT_NORM, false>, dissect_all<PRINT_LESS, false>, dissect_all<PRINT_HEX, false> },
		{ dissect_all<PRINT_NORM, true>, dissect_all<PRINT_LESS, true>, dissect_all<PRINT_HEX, true> },
	};
	// compact records of walker-heavy batches: the record ring's build (an
	// instantiation of its own: beside the ring's code, the records held one
	// tile in registers spill, and without them C3 runs 4 % slower)
	static const kfn ring_kernels[2] = { dissect_all<PRINT_NORM, true, true>,
					     dissect_all<PRINT_LESS, true, true> };
	return ring ? ring_kernels[mi] : kernels[compact][mi];
}

ffn fast_kernel(bool compact, int mi)
{
	static const ffn fast[2][3] = {
		{ dissect_fast<PRINT_NORM, false>, dissect_fast<PRINT_LESS, false>, dissect_fast<PRINT_HEX, false> },
		{ dissect_fast<PRINT_NORM, true>, dissect_fast<PRINT_LESS, true>, dissect_fast<PRINT_HEX, true> },
	};
	return fast[compact][mi];
}

void (*zero_tiles_kernel())(uint32_t *, uint32_t)
{
	return zero_tiles;
}

} // namespace nsd
