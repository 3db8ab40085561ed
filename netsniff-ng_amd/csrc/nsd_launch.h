// nsd_launch.h - what the kernels (nsd_kernels.hip) and their launcher
// (nsd_launch.hip) must agree on: the tunables, the block shape, the strides
// and sizes of what a launch keeps in its workspace and in a tail counter
// set, the kernels' types, and the workspace layout (ws_layout: the one place
// that computes it).
#ifndef NSD_LAUNCH_H
#define NSD_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nsd_internal.h"

// ---- numeric tunables (each overridable with -D: tools/build_variant.sh) -----
#ifndef NSD_WIN2
#define NSD_WIN2 128               // bytes per staged window of the general walk's continuation
#endif
#ifndef NSD_CSUM_U
#define NSD_CSUM_U 12              // interior chunk loads in flight per lane (icmp_pass)
#endif
#ifndef NSD_FAST_CSUM_U
#define NSD_FAST_CSUM_U 8          // the same in fast_icmp_pass (4: C3 split +4 %)
#endif
#ifndef NSD_CSUM_LANES
#define NSD_CSUM_LANES 8           // lanes per message in icmp_pass (each group instruction: 8 = one 128-B line)
#endif
#ifndef NSD_MINW
#define NSD_MINW 4                 // waves per SIMD the fused kernel is register-allocated for
#endif
#ifndef NSD_FAST_MINW
#define NSD_FAST_MINW 4            // waves per SIMD dissect_fast is register-allocated for (compact records)
#endif
#ifndef NSD_FAST_MINW_FULL
#define NSD_FAST_MINW_FULL 4       // the same for 16-byte records (the deferral entries carry layer starts)
#endif
#ifndef NSD_FAST_BPC
#define NSD_FAST_BPC 3             // resident fast blocks per CU (0: as many as fit)
#endif
#ifndef NSD_FAST_BPC_SMALL
#define NSD_FAST_BPC_SMALL 2       // the same when the sampled frames average at most NSD_SMALL_FRAME bytes
#endif
#ifndef NSD_GROUP_BLOCKS
#define NSD_GROUP_BLOCKS 4u        // blocks sharing a tile counter (4: one CU's; 8: two CUs of one XCD)
#endif
#ifndef NSD_L2PF
#define NSD_L2PF 16                // a tile with this many deferred packets is walker-heavy (walk_tiles' `late`)
#endif
#ifndef NSD_REFILL
#define NSD_REFILL 16              // idle walkers at which a session stops to take waiting packets (walkers)
#endif
#ifndef NSD_WIN_AHEAD
#define NSD_WIN_AHEAD 32           // bytes a walker's window keeps past the next layer's in its last line (window_len)
#endif
#ifndef NSD_SCHED_SAMPLE
#define NSD_SCHED_SAMPLE 32        // launches on a device between two schedule samples (sched_plan)
#endif
#ifndef NSD_TAIL_DIV
#define NSD_TAIL_DIV 2             // the fast kernel shares the last 1 / NSD_TAIL_DIV of its rounds at run time (0: none)
#endif
#ifndef NSD_TAIL_MIN_ROUNDS
#define NSD_TAIL_MIN_ROUNDS 16     // rounds (a wave's share of tiles) below which every tile is static
#endif
#ifndef NSD_TAIL_HEAD_BLOCKS
#define NSD_TAIL_HEAD_BLOCKS 16    // blocks per head of the shared tail (64 waves a head; at least 4: fast_tiles' liveness)
#endif
#ifndef NSD_TAIL_TRIES
#define NSD_TAIL_TRIES 3u          // other heads a wave tries once its own is empty
#endif
#ifndef NSD_SMALL_FRAME
#define NSD_SMALL_FRAME 128        // average frame bytes up to which a sampled batch counts as small frames
#endif

// A persistent grid of at most NSD_MAX_GRID blocks; block b owns pending
// lists b (room for every packet it visits).
constexpr uint32_t NSD_MAX_GRID = 4096;
// heads of a tail counter set at most (tail_set; WsLayout::tail_heads)
constexpr uint32_t NSD_TAIL_HEADS_MAX = 256;

namespace nsd {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;

// a slot of a fast wave's list (dissect_fast): SW uint4
constexpr int SW = 2;
constexpr int LIST_SLOT_BYTES = SW * 16;
// an entry of a pending list (pend_entry, leaf_entry): a u64
constexpr int PEND_BYTES = 8;
// every counter the waves of several blocks draw from has a 128-byte line of
// its own, as word 0 of LINE_WORDS: the fused kernel's group tile counters
// (walk_tiles, zero_tiles), the shared tail's heads and, after the last
// head, the word that counts the blocks done (fast_tiles, dissect_fast)
constexpr int LINE_BYTES = 128;
constexpr int LINE_WORDS = LINE_BYTES / 4;
// The fused kernel's pending-list slots per block, from the packets a block
// visits at an even share (`region`).  Compact records: its waves take their
// group's tiles at run time (walk_tiles), so each list holds twice a wave's
// even share plus four tiles.  (Each packet a wave visits adds at most one
// pending-list entry - an ICMPv4 message past its windows from the front, or
// a host-rendered leaf from the back, never both: a leaf ends a chain that
// has no ICMPv4 layer - and walk_tiles asks for a tile only while the list
// has room for every packet of the tiles it holds; a wave that found its
// list overrun counts it in NSD_CNT_LISTOVF.)
constexpr uint32_t fused_region(uint32_t region, bool compact)
{
	return compact ? 2 * region + WAVES * 4 * 64 : region;
}
// the schedule sample's pair (sched_plan): two u64 the kernels add to
constexpr int PAIR_BYTES = 16;
// with a shared tail a wave may walk more than its share: its lists hold
// 1 / TAIL_CAP_DIV more slots (WsLayout::sh; fast_tiles' liveness)
constexpr uint32_t TAIL_CAP_DIV = 5;

// ---- the kernels (nsd_kernels.hip) --------------------------------------------
typedef void (*kfn)(const uint8_t *, const uint64_t *, uint32_t, int, void *, uint32_t *, uint32_t, uint32_t *,
		    uint32_t, unsigned long long *, uint64_t *, uint32_t, const uint32_t *, unsigned long long *,
		    uint32_t *, uint32_t);
typedef void (*ffn)(const uint8_t *, const uint64_t *, uint32_t, int, void *, unsigned long long *, uint4 *,
		    uint32_t, const uint32_t *, uint32_t *, unsigned long long *, uint32_t *, uint32_t, uint32_t *,
		    uint32_t, uint64_t *, uint32_t, uint32_t *, uint32_t, uint32_t);
// mi: 0 PRINT_NORM, 1 PRINT_LESS, 2 every other mode (no chain).  ring: the
// record ring's build of dissect_all (compact records, mi < 2 only)
NSD_HIDDEN kfn fused_kernel(bool compact, int mi, bool ring);
NSD_HIDDEN ffn fast_kernel(bool compact, int mi);
NSD_HIDDEN void (*zero_tiles_kernel())(uint32_t *, uint32_t);

// ---- the workspace of one launch (nsd_launch.hip) -----------------------------
// Where a launch of n packets on a grid of `blocks` keeps what, as byte
// offsets from the workspace's start.  The fused kernel's pending lists and
// the split schedule's lists both start at 0 (a launch runs one of them).
struct WsLayout {
	// the grid: one block per BLOCK packets at most, and NSD_MAX_GRID
	uint32_t blocks;
	// a wave's share of tiles (a block visits rounds * BLOCK packets)
	uint32_t rounds;
	// The split schedule's carve: per wave a fast list of `cap` slots from
	// the start, then PEND_BYTES no kernel uses per list (the size callers
	// allocate is kept), then the tail's pending lists at pend_at, `cap`
	// entries per wave (a packet the tail walks adds at most one).
	struct Carve {
		uint32_t cap;
		size_t lists_bytes, pend_at, pend_bytes;
	};
	// st, static tiles: cap is the wave's share.  sh, a shared tail: a fifth
	// more, in the same bytes - the workspace keeps 32 + 16 bytes per packet
	// slot below the tile counters and the static carve uses 32 + 8 of them;
	// 1.2 x (32 + 8) = 48.
	Carve st, sh;
	// sh ends at or below gtiles_at (a grid near NSD_MAX_GRID can miss it by
	// the alignment; such a launch runs the static loop)
	bool sh_fits;
	// the fused kernel's pending-list slots per block (fused_region)
	uint32_t fused_region;
	// the fused kernel's group tile counters (a line per block at most), then
	// the schedule sample's pair in the last 256 bytes; both depend on n alone
	size_t gtiles_at, pair_at, total;
	// The shared tail: the rounds it shares (0: every tile is static; rounds
	// below NSD_TAIL_MIN_ROUNDS, or sh does not fit) and its heads.
	// fast_tiles' liveness: a wave stopped for room has walked rounds +
	// rounds / 5 - 1 tiles or more, i.e. y + rounds / 5 - 1 of the tail's (y
	// shared rounds, at most rounds / 2 + 1), and a head's tiles are at most
	// 17 / 16 of y per home wave (16 blocks a head or more): y + rounds / 5 -
	// 1 > y * 17 / 16 for every rounds >= 16 while y <= rounds / 2 + 1
	uint32_t tail_rounds, tail_heads;
};
NSD_HIDDEN WsLayout ws_layout(uint32_t n, uint32_t blocks, bool compact);

} // namespace nsd

#endif
