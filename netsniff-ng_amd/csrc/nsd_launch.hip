// nsd_launch.hip - the launcher of the dissect kernels (C ABI, called by
// nsd_host.cpp / nsd_pipe.cpp): the adaptive schedule, the shared tail's
// counter sets, the nsd_set_* switches, the workspace layout (ws_layout) and
// nsd_launch_dissect_rec.  The kernels are nsd_kernels.hip's; what both files
// agree on is in nsd_launch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "nsd_internal.h"
#include "nsd_launch.h"

// ---- the schedule -------------------------------------------------------------
// split (dissect_fast) or fused (dissect_all), one launch either way.  The
// split schedule runs a fast loop with two tiles in flight per wave and
// none of the walker pool's state, and wins when the fast walk finishes
// nearly every packet and few ICMPv4 messages run past their windows (C2
// 16M x 64 B: 0.233 against 0.249 ms).  When many packets need the general
// walk (C4's IPv6 extension chains) the fused kernel wins by far (1.17
// against 1.88 ms): its walkers take a tile's packets while their first
// lines are still on chip, where the split schedule's tail re-reads them
// and its fast loop writes a list entry per packet.
// When many ICMPv4 checksums are left to a pass (C3 IMIX: about a fifth of
// the packets) the fused kernel wins too (0.70 - 0.75 against 0.73 - 0.81
// ms on the same boxes, r03): its checksum pass streams at 4 waves per SIMD
// with 8 loads in flight per lane.  Adaptive (the default): every
// NSD_SCHED_SAMPLE launches on a device, one launch is sampled: its kernels
// count the packets the fast walk handed over and the ICMPv4 messages left
// to a pass into a pair at the end of that launch's own workspace (zeroed
// before it, copied to pinned host memory after it, on its stream), so
// launches on other streams or pipes never mix into the sample.  Once the
// copy has landed, the two shares of that launch's packets pick the
// schedule for the launches after it, with hysteresis (fused above 15 %
// deferred or 10 % pending checksums, split again below 5 % of both).  A
// capture's traffic mix changes slowly against batches of a few
// milliseconds; both schedules give identical results.  nsd_set_schedule
// forces one (tests).  The same sample brings back the launch's packet and
// byte counts (the counter vector before and after it): when its frames
// average at most NSD_SMALL_FRAME bytes, the fast kernel runs
// NSD_FAST_BPC_SMALL blocks per CU instead of NSD_FAST_BPC (C2's 64-byte
// frames stream from few waves: 0.217 -> 0.207 ms at 2 blocks per CU on one
// box, where IMIX frames need the third: 0.78 against 0.92 ms); and when
// more than a quarter of its packets went to the walkers, the fused kernel
// runs without the progress priority (walk_tiles: C4 -1 % without it, C3
// +0.7 %, in the same kernel) and with the record ring (RingSt: C4's writes
// halved, C3 +3 % with it; on until the first sample is read).  State is per
// device.
namespace {
constexpr int MAX_DEV = 16;
struct Sched {
	bool init = false, fused = false, pending = false, small = false;
	bool walky = false;                    // the sample's deferred share above 25 % (no progress priority)
	bool sampled_once = false;             // a sample has been read
	bool recorded = false;                 // the pending sample's event is recorded (sched_sampled)
	bool discard = false;                  // the pending sample failed: wait for its copies, use nothing
	int launches = 0;
	int last = 0;                          // the last launch's schedule (nsd_last_schedule)
	bool last_shared = false;              // the last launch's fast kernel shared its tail (nsd_last_tail_shared)
	uint64_t sampled = 0;                  // packets of the sampled launch in flight
	unsigned long long *host = nullptr;    // its pair, then its counters [32, 34) before and after
	hipEvent_t ev = nullptr;
	int cus = 0;                           // compute units of the device
};
Sched g_sched[MAX_DEV];
std::mutex g_sched_mu;
int g_sched_force = 0;   // 0 adaptive, NSD_SCHED_SPLIT, NSD_SCHED_FUSED
int g_ring_force = 0;    // nsd_set_record_ring: 0 adaptive, 1 on, 2 off
std::atomic<int> g_grid_cap{ 0 };   // nsd_set_grid_cap
std::atomic<int> g_debug_fill{ -1 };   // nsd_set_debug_fill: -1 off, else the byte

int cur_dev()
{
	int d = 0;
	if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEV)
		d = 0;
	return d;
}

// The plan of one launch of n packets on the current device: the schedule,
// and whether this launch is the sample (then its pair is zeroed on
// `stream` here and copied back by sched_sampled after the kernels).
// capturing: `stream` is capturing into a graph.
struct Plan {
	bool fused, sample, small, prio, ring;
	int cus;
};
Plan sched_plan(uint32_t n, unsigned long long *pair, const uint64_t *counters, hipStream_t stream, bool capturing)
{
	std::lock_guard<std::mutex> g(g_sched_mu);
	const int dev = cur_dev();
	Sched &S = g_sched[dev];
	if (!S.cus) {
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
			cus = 256;
		S.cus = cus;
	}
	Plan p{ false, false, false, true, true, S.cus };
	// a launch captured into a graph takes the schedule as it stands and is
	// never the sample (an event query or a host copy would break the
	// capture; the graph replays this plan)
	// (a sample is read only once sched_sampled has recorded its event: between
	// the plan and that record, the event still stands for an older sample, and
	// another stream's launch must not take the copies in flight for it).
	// One query: an event that completed between two would let a failed
	// sample's half-landed words pass for a sample.
	const bool landed = !capturing && S.pending && S.recorded && hipEventQuery(S.ev) == hipSuccess;
	if (landed && S.discard) {
		S.pending = S.recorded = S.discard = false;
	} else if (landed) {
		const double rd = S.sampled ? (double)S.host[0] / (double)S.sampled : 0.0;
		const double ri = S.sampled ? (double)S.host[1] / (double)S.sampled : 0.0;
		S.fused = S.fused ? rd > 0.05 || ri > 0.05 : rd > 0.15 || ri > 0.10;
		const uint64_t pk = S.host[4] - S.host[2], by = S.host[5] - S.host[3];
		if (pk)
			S.small = by <= (uint64_t)NSD_SMALL_FRAME * pk;
		S.walky = rd > 0.25;
		S.sampled_once = true;
		S.pending = false;
		S.recorded = false;
	}
	if (!S.init && !capturing) {
		S.init = true;
		if (hipHostMalloc((void **)&S.host, 64, hipHostMallocDefault) != hipSuccess ||
		    hipEventCreateWithFlags(&S.ev, hipEventDisableTiming) != hipSuccess)
			S.host = nullptr;
	}
	p.fused = g_sched_force ? g_sched_force == NSD_SCHED_FUSED : S.fused;
	p.small = S.small;
	p.prio = !S.walky;
	// the record ring until a sample shows a quarter or less of the packets
	// deferred (C3: +3 % with it; C4: writes 23.7 -> 12.2 B/packet)
	p.ring = g_ring_force ? g_ring_force == 1 : !S.sampled_once || S.walky;
	if (!capturing && ++S.launches >= NSD_SCHED_SAMPLE && !S.pending && S.host && pair && counters &&
	    hipMemsetAsync(pair, 0, nsd::PAIR_BYTES, stream) == hipSuccess &&
	    hipMemcpyAsync(S.host + 2, counters + NSD_CNT_PKTS, 16, hipMemcpyDeviceToHost, stream) == hipSuccess) {
		p.sample = true;
		S.launches = 0;
		S.sampled = n;
		S.pending = true;   // (until its copy lands)
		S.recorded = false;
	}
	return p;
}

// what the launch that was just queued runs, for nsd_last_schedule and
// nsd_last_tail_shared
void sched_ran(bool fused, bool shared)
{
	std::lock_guard<std::mutex> g(g_sched_mu);
	Sched &S = g_sched[cur_dev()];
	S.last = fused ? NSD_SCHED_FUSED : NSD_SCHED_SPLIT;
	S.last_shared = shared;
}

// The fast kernel's shared tail draws its tiles from heads that are zero
// between launches (fast_tiles, dissect_fast).  They live in counter sets the
// library owns, one per (device, stream), not in the caller's workspace: a
// workspace comes as it is (torch.empty, the debug fill), and zeroing words of
// it would cost a launch or a memset per batch.  A set is made on its
// stream's first launch - zeroed once, on that stream - and never freed (as
// Sched::host); the kernel leaves it zeroed, and launches on one stream are
// ordered.  One 128-byte line per head, then the line of the blocks' count.
// nullptr (the static loop): allocation failed, or NSD_TAIL_SETS streams have
// one already.
constexpr int NSD_TAIL_SETS = 64;
struct TailSet {
	int dev;
	hipStream_t stream;
	uint32_t *heads;
};
TailSet g_tail[NSD_TAIL_SETS];
int g_ntail = 0;

uint32_t *tail_set(hipStream_t stream)
{
	// (hipStreamPerThread names a different stream in every thread: no set)
	if (stream == hipStreamPerThread)
		return nullptr;
	std::lock_guard<std::mutex> g(g_sched_mu);
	const int dev = cur_dev();
	for (int k = 0; k < g_ntail; k++)
		if (g_tail[k].dev == dev && g_tail[k].stream == stream)
			return g_tail[k].heads;
	if (g_ntail == NSD_TAIL_SETS)
		return nullptr;
	const size_t bytes = (size_t)(NSD_TAIL_HEADS_MAX + 1) * nsd::LINE_BYTES;
	uint32_t *h = nullptr;
	if (hipMalloc((void **)&h, bytes) != hipSuccess) {
		(void)hipGetLastError();
		return nullptr;
	}
	if (hipMemsetAsync(h, 0, bytes, stream) != hipSuccess) {
		(void)hipGetLastError();
		(void)hipFree(h);
		return nullptr;
	}
	g_tail[g_ntail++] = TailSet{ dev, stream, h };
	return h;
}

// A failed sample (under the lock): copies queued for it may still be in
// flight into S.host, so the sample stays pending - no later sample queues
// copies into the same words - until an event behind them completes, and
// its values are discarded then (sched_plan).  Without an event, the stream
// is drained here instead.
void sched_fail(Sched &S, hipStream_t stream)
{
	S.discard = true;
	if (hipEventRecord(S.ev, stream) == hipSuccess) {
		S.recorded = true;
		return;
	}
	(void)hipStreamSynchronize(stream);
	S.pending = S.recorded = S.discard = false;
}

// after the sampled launch's kernels on `stream`: bring its pair and
// counters back
void sched_sampled(unsigned long long *pair, const uint64_t *counters, hipStream_t stream)
{
	std::lock_guard<std::mutex> g(g_sched_mu);
	Sched &S = g_sched[cur_dev()];
	if (hipMemcpyAsync(S.host, pair, nsd::PAIR_BYTES, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipMemcpyAsync(S.host + 4, counters + NSD_CNT_PKTS, 16, hipMemcpyDeviceToHost, stream) != hipSuccess ||
	    hipEventRecord(S.ev, stream) != hipSuccess) {
		sched_fail(S, stream);
		return;
	}
	S.recorded = true;
}

// the sampled launch's kernels failed to launch: drop the sample (once the
// copies sched_plan queued for it have landed)
void sched_abort(hipStream_t stream)
{
	std::lock_guard<std::mutex> g(g_sched_mu);
	sched_fail(g_sched[cur_dev()], stream);
}
} // namespace

extern "C" int nsd_set_schedule(int sched)
{
	if (sched != NSD_SCHED_ADAPTIVE && sched != NSD_SCHED_SPLIT && sched != NSD_SCHED_FUSED)
		return NSD_ERR_ARG;
	std::lock_guard<std::mutex> g(g_sched_mu);
	const int prev = g_sched_force;
	g_sched_force = sched;
	return prev;
}

extern "C" int nsd_set_record_ring(int mode)
{
	if (mode < 0 || mode > 2)
		return NSD_ERR_ARG;
	std::lock_guard<std::mutex> g(g_sched_mu);
	const int prev = g_ring_force;
	g_ring_force = mode;
	return prev;
}

extern "C" int nsd_set_grid_cap(int blocks)
{
	if (blocks < 0)
		return NSD_ERR_ARG;
	return g_grid_cap.exchange(blocks);
}

extern "C" int nsd_set_debug_fill(int byte)
{
	if (byte < -1 || byte > 255)
		return NSD_ERR_ARG;
	return g_debug_fill.exchange(byte);
}

// 1 when the last launch on the current device ran dissect_fast with a shared
// tail (tickets from a counter set), 0 when its tiles were static or it ran
// the fused kernel (tests)
extern "C" int nsd_last_tail_shared(void)
{
	std::lock_guard<std::mutex> g(g_sched_mu);
	return g_sched[cur_dev()].last_shared ? 1 : 0;
}

extern "C" int nsd_last_schedule(void)
{
	std::lock_guard<std::mutex> g(g_sched_mu);
	return g_sched[cur_dev()].last;
}

// ---- the workspace ------------------------------------------------------------
static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static_assert(NSD_TAIL_DIV == 0 || (NSD_TAIL_DIV >= 2 && NSD_TAIL_MIN_ROUNDS >= 16 && NSD_TAIL_HEAD_BLOCKS >= 16),
	      "fast_tiles: a static front of more than three rounds, and its liveness argument");

// (the fields' reasons: nsd_launch.h)
nsd::WsLayout nsd::ws_layout(uint32_t n, uint32_t blocks, bool compact)
{
	WsLayout L;
	const uint32_t want = ((n + 63) / 64 + WAVES - 1) / WAVES;
	if (blocks > NSD_MAX_GRID)
		blocks = NSD_MAX_GRID;
	L.blocks = blocks < want ? blocks : want;
	const uint64_t stride = (uint64_t)L.blocks * BLOCK;
	L.rounds = (uint32_t)((n + stride - 1) / stride);
	// Sized for the worst case over grids (the sum of the blocks' shares is at
	// most n + blocks * BLOCK packet slots): LIST_SLOT_BYTES a slot for the
	// fast lists, the lists' unused PEND_BYTES, two pending entries' bytes a
	// slot (the static carve uses one; the fused kernel's lists, PEND_BYTES a
	// slot, lie within the first LIST_SLOT_BYTES a slot).
	const size_t slots = ((size_t)n + (size_t)NSD_MAX_GRID * BLOCK + 1) & ~(size_t)1;
	L.gtiles_at = align256(align256(LIST_SLOT_BYTES * slots) + align256((size_t)NSD_MAX_GRID * WAVES * PEND_BYTES) +
			       2 * PEND_BYTES * slots);
	L.pair_at = L.gtiles_at + (size_t)NSD_MAX_GRID * LINE_BYTES;
	L.total = L.pair_at + 256;
	const size_t nlists = (size_t)L.blocks * WAVES;
	auto carve = [&](uint32_t cap) {
		const size_t lists_bytes = LIST_SLOT_BYTES * nlists * cap;
		return WsLayout::Carve{ cap, lists_bytes, align256(lists_bytes) + align256(nlists * PEND_BYTES),
					PEND_BYTES * nlists * cap };
	};
	L.st = carve(L.rounds * 64);
	L.sh = carve(L.st.cap + L.st.cap / TAIL_CAP_DIV);
	L.sh_fits = L.sh.pend_at + L.sh.pend_bytes <= L.gtiles_at;
	L.fused_region = fused_region(L.rounds * BLOCK, compact);
	L.tail_rounds = 0;
	if (NSD_TAIL_DIV != 0 && L.sh_fits && L.rounds >= NSD_TAIL_MIN_ROUNDS) {
		uint32_t t = L.rounds / NSD_TAIL_DIV;
		if (!t)
			t = 1;
		// (an even front: a ticket's pair then falls on one turn of the unrolled loop)
		L.tail_rounds = t + ((L.rounds - t) & 1);
	}
	uint32_t h = L.blocks / NSD_TAIL_HEAD_BLOCKS;
	if (h >= 8)
		h &= ~7u;   // whole XCDs' worth: a head's blocks share blockIdx.x % 8
	if (h > NSD_TAIL_HEADS_MAX)
		h = NSD_TAIL_HEADS_MAX & ~7u;
	L.tail_heads = h ? h : 1;
	return L;
}

extern "C" size_t nsd_launch_workspace_bytes(uint32_t n)
{
	return nsd::ws_layout(n, 1, false).total;
}

// ws_layout(n, blocks, compact) as byte offsets and extents, for tests:
//   out[0]      nsd_launch_workspace_bytes(n)
//   out[1, 2]   the fused kernel's pending lists (8 bytes a slot)
//   out[3, 4]   its tile counters (a 128-byte line per block; compact only: else extent 0)
//   out[5, 6]   the schedule sample's pair
//   out[7, 8]   the split schedule's fast lists, static tiles (32 bytes a slot)
//   out[9, 10]  its tail's pending lists, static tiles
//   out[11, 12] the fast lists with a shared tail
//   out[13, 14] the pending lists with a shared tail
//   out[15]     1 when the carve with a shared tail fits (else such a launch is static)
//   out[16, 17] a wave's list slots, static and with a shared tail
//   out[18, 19] the shared tail's rounds (0: the launch is static) and heads
extern "C" int nsd_launch_workspace_layout(uint32_t n, uint32_t blocks, int compact, uint64_t *out)
{
	if (!n || !blocks || !out)
		return NSD_ERR_ARG;
	const nsd::WsLayout L = nsd::ws_layout(n, blocks, compact != 0);
	const uint64_t v[20] = { L.total, 0, (uint64_t)nsd::PEND_BYTES * L.fused_region * L.blocks,
				 L.gtiles_at, compact ? (uint64_t)nsd::LINE_BYTES * L.blocks : 0,
				 L.pair_at, (uint64_t)nsd::PAIR_BYTES,
				 0, L.st.lists_bytes, L.st.pend_at, L.st.pend_bytes,
				 0, L.sh.lists_bytes, L.sh.pend_at, L.sh.pend_bytes,
				 L.sh_fits, L.st.cap, L.sh.cap, L.tail_rounds, L.tail_heads };
	for (int k = 0; k < 20; k++)
		out[k] = v[k];
	return 0;
}

// d_sll: one struct sockaddr_ll (nsd_sll_t, 20 bytes) per packet, or NULL
// (read as zeros); used by the LINKTYPE_LINUX_SLL head only.  d_rec: n
// nsd_rec (16 B), or n nsd_crec (8 B) when `compact`.
extern "C" int nsd_launch_dissect_rec(const uint8_t *d_frames, const uint64_t *d_desc, const void *d_sll,
				      uint32_t n, int start_id, int mode, void *d_rec, int compact, uint32_t *d_ext,
				      uint32_t ext_words, uint32_t *d_ext_used, uint64_t *d_counters, void *d_ws,
				      int grid, hipStream_t stream)
{
	using namespace nsd;
	if (n == 0)
		return 0;
	const int mi = mode == PRINT_NORM ? 0 : mode == PRINT_LESS ? 1 : 2;
	const int ci = compact ? 1 : 0;
	// ext pool chunk per request: half the pool spread over the waves, so the
	// unused chunk tails the waves keep at the end waste at most half of it
	// (a pool of 2x the words the chains need never overflows), within
	// [1 deep entry, 512 short entries]
	if (ext_words > NSD_EXT_POOL_MAX_WORDS)
		ext_words = NSD_EXT_POOL_MAX_WORDS;
	auto chunk_for = [&](uint32_t blocks) {
		const uint64_t per = (uint64_t)ext_words / (2ull * blocks * WAVES);
		const uint32_t lo = NSD_EXT_WORDS(NSD_EXT_MAX_LAYERS), hi = 512 * NSD_EXT_WORDS(16);
		return (uint32_t)(per < lo ? lo : per > hi ? hi : per) & ~3u;
	};
	// persistent grids: exactly the blocks that are resident together (CUs x
	// the kernel's occupancy), so no block waits for a second round; every
	// block grid-strides (counters then cost one flush per block).  The
	// occupancy of a kernel is a property of its code (one gfx950 build):
	// cached once, racing callers store the same value.
	auto occupancy = [&](const void *f, std::atomic<int> &slot, int dflt) {
		int occ = slot.load(std::memory_order_relaxed);
		if (!occ) {
			if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, f, BLOCK, 0) != hipSuccess || occ < 1)
				occ = dflt;
			slot.store(occ, std::memory_order_relaxed);
		}
		return occ;
	};
	if (grid <= 0)
		grid = g_grid_cap.load(std::memory_order_relaxed);
	// the one capture query of the launch, for the debug fill, the plan and the tail
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	const bool cs_known = hipStreamIsCapturing(stream, &cs) == hipSuccess;
	const bool capturing = cs_known && cs != hipStreamCaptureStatusNone;
	// total and pair_at depend on n alone (the grid comes with the plan, below)
	const WsLayout L0 = ws_layout(n, 1, compact != 0);
	// nsd_set_debug_fill (tests): everything this launch is about to write -
	// records, pool, workspace - filled with the byte first, ahead of all the
	// launch queues (the sample's pair memset, zero_tiles, the kernels), so a
	// store that never happens leaves the fill and not an earlier launch's
	// value.  Not into a capturing stream (a graph replays its own nodes
	// only; the caller fills before a replay).  ext_used and the counters
	// accumulate and stay.
	const int fill = g_debug_fill.load(std::memory_order_relaxed);
	if (fill >= 0 && cs_known && !capturing) {
		if (hipMemsetAsync(d_rec, fill, (size_t)n * (compact ? sizeof(nsd_crec) : sizeof(nsd_rec)), stream) != hipSuccess ||
		    (d_ext && ext_words && hipMemsetAsync(d_ext, fill, (size_t)ext_words * 4, stream) != hipSuccess) ||
		    (d_ws && hipMemsetAsync(d_ws, fill, L0.total, stream) != hipSuccess))
			return -2;
	}
	uint8_t *const ws = (uint8_t *)d_ws;
	unsigned long long *const pair = ws ? (unsigned long long *)(ws + L0.pair_at) : nullptr;
	const Plan plan = sched_plan(n, mi != 2 ? pair : nullptr, d_counters, stream, capturing);
	const int s_cus = plan.cus;
	unsigned long long *const sched = plan.sample ? pair : nullptr;
	// after a kernel launch: a launch error drops the sample and fails the call
	auto launched = [&]() {
		if (hipGetLastError() == hipSuccess)
			return true;
		if (sched)
			sched_abort(stream);
		return false;
	};
	uint32_t *heads = nullptr;   // the split schedule's shared tail: its counter set
	if (mi != 2 && plan.fused) {
		static std::atomic<int> s_occ[2][3], s_rocc[2];
		const bool ring = plan.ring && ci == 1 && mi < 2;
		const kfn f = fused_kernel(ci, mi, ring);
		std::atomic<int> &occ_slot = ring ? s_rocc[mi] : s_occ[ci][mi];
		const WsLayout L = ws_layout(n, grid > 0 ? (uint32_t)grid : (uint32_t)(s_cus * occupancy((const void *)f, occ_slot, 4)),
					     compact != 0);
		// the CU groups' tile counters (walk_tiles), a line each, zeroed on the
		// launch's stream
		uint32_t *const gtiles = (uint32_t *)(ws + L.gtiles_at);
		if (compact) {
			hipLaunchKernelGGL(zero_tiles_kernel(), dim3((L.blocks + 255) / 256), dim3(256), 0, stream, gtiles,
					   L.blocks);
			if (!launched())
				return -2;
		}
		hipLaunchKernelGGL(f, dim3(L.blocks), dim3(BLOCK), 0, stream, d_frames, d_desc, n, start_id, d_rec, d_ext,
				   ext_words, d_ext_used, chunk_for(L.blocks), (unsigned long long *)d_counters,
				   (uint64_t *)ws, L.fused_region, (const uint32_t *)d_sll, sched, gtiles,
				   plan.prio ? 1u : 0u);
	} else {
		static std::atomic<int> s_focc[2][3];
		const ffn f = fast_kernel(ci, mi);
		// grid > 0 (tests): the grid capped at `grid` blocks
		uint32_t fcap = grid > 0 ? (uint32_t)grid : (uint32_t)(s_cus * occupancy((const void *)f, s_focc[ci][mi], 8));
		// with two tiles in flight per wave, 3 blocks per CU outrun the 4 that
		// fit (HBM serves fewer concurrent streams better), and 2
		// the 3 when the frames are small (the sample, sched_plan)
		const int bpc = plan.small ? NSD_FAST_BPC_SMALL : NSD_FAST_BPC;
		if (grid <= 0 && bpc > 0 && fcap > (uint32_t)(s_cus * bpc))
			fcap = (uint32_t)(s_cus * bpc);
		const WsLayout L = ws_layout(n, fcap, compact != 0);
		// The last rounds' tiles handed out at run time (fast_tiles), when the
		// launch has rounds enough, its lists fit a fifth larger (L.tail_rounds)
		// and the stream has a counter set; not in a capture (a graph replays
		// its arguments on whatever stream it is launched into) and not for
		// the modes without a chain.  Else every tile is static.
		const uint32_t trounds = mi != 2 && !capturing ? L.tail_rounds : 0;
		heads = trounds ? tail_set(stream) : nullptr;
		const WsLayout::Carve &cv = heads ? L.sh : L.st;
		const uint32_t tail0 = heads ? (L.rounds - trounds) * L.blocks * WAVES : 0;
		// compact records: the pool's side words (when it has them), for leaf ends
		uint32_t *side = compact && d_ext && ext_words >= n ? d_ext : nullptr;
		hipLaunchKernelGGL(f, dim3(L.blocks), dim3(BLOCK), 0, stream, d_frames, d_desc, n, start_id, d_rec,
				   (unsigned long long *)d_counters, (uint4 *)ws, cv.cap, (const uint32_t *)d_sll, side, sched,
				   d_ext, ext_words, d_ext_used, chunk_for(L.blocks), (uint64_t *)(ws + cv.pend_at),
				   cv.cap * WAVES, heads, tail0, L.tail_heads);
	}
	if (!launched())
		return -2;
	sched_ran(plan.fused, heads != nullptr);
	if (sched)
		sched_sampled(sched, d_counters, stream);
	return 0;
}
