// nsd_fused.h - the fused kernel (dissect_all) and the walker pool, which
// the split kernel's tail runs too (walk_lists, nsd_fast.h).
#ifndef NSD_FUSED_H
#define NSD_FUSED_H

#include "nsd_stage.h"

namespace nsd {

// ---- the fused kernel ---------------------------------------------------------
// Block-level shared state of one dissect launch.
// a wave's window area: the fast walk's 20-dword rows, then (same words) the
// continuation's WIN2-byte rows
constexpr int WINWORDS = 64 * row_of(WIN1) > 16 * WIN2 ? 64 * row_of(WIN1) : 16 * WIN2;
struct Shared {
	alignas(16) uint32_t win[WAVES][WINWORDS];              // staged windows (fast walk, then continuations)
	unsigned long long cnt[NSD_NCOUNTERS];      // block counters
	uint32_t ops[32];                           // block per-ops layer counts (32-bit LDS atomics)
	uint8_t lay3[256];                          // eth_lay3
	uint32_t step[64];                          // c_step, c_lay2h (general walk)
	uint32_t wc[WAVES][2];                      // per-wave ext pool chunk {next word, words left}
	uint32_t pcnt[WAVES];                       // pending checksums per wave
	// general-walk layer lists (layers 6..11, 16-byte records); compact
	// records keep no layer starts, and the fused kernel's waves use the
	// words as their record rings (RecRing)
	alignas(16) uint32_t lay[WAVES][NSD_LDS_LAYERS * 64];
	uint8_t tmap[WAVES][64];                    // take(): pending lane of each rank
};

// The fused kernel's record ring (compact records of walker-heavy batches:
// a build of its own, dissect_all<MODE, true, true>, which the launcher runs
// when the schedule sample defers more than a quarter of the packets; the
// plain build holds a tile's records one tile in registers, HeldSt, which do
// not fit beside the ring's code: 11 VGPRs spilled, C3 +28 %, and stored
// right after the fast walk instead C3 ran 4 % slower).  In the ring build
// a tile whose packets the fast walk all finishes stores its records at
// once, right after its fast walk.  A tile with deferred packets has its
// records written
// twice over: by the fast walk (the packets it finishes) and later by the
// walkers' sessions (each session's finished packets), often across two
// tiles.  Stored to HBM as they came, a 128-byte line of records (16
// packets) was written in two or three pieces microseconds apart, and the
// XCD's L2 had let the line go in between, so each piece cost its own
// partial-line writes (C4: 17.4 B/packet written for 8 B of records, and
// 6.3 more for the side words' 4-byte stores; TCC_EA0_WRREQ: 37 % of the
// requests 32-byte ones).  Here each wave keeps two such tiles' records and
// side words in LDS (the compact form's unused layer-list words: 2 x 64 x 8
// B + 2 x 64 x 4 B = 1,536 B a wave) and stores a tile's records in one
// coalesced wave store (512 B, whole lines) once its last packet is
// finished; its side words likewise (256 B) when any packet of the tile has
// one (C4), zero for the tile's packets without one.  A slot needed by a new
// tile while packets of its old tile are still held by walkers (walked
// across two more tiles) stores the finished ones at once, and those
// walkers store theirs directly (the tile has left the ring).  The state is
// wave-uniform and lives in scalar registers (a round trip to LDS for it
// before each tile's prefetch loads cost 5 %).  C4: 23.7 -> 12.2 B/packet
// written per launch, kernel time within the box's noise (+-1 %: C4's
// walker steps, not its bytes, set its time).
constexpr uint32_t RING_NONE = 0xFFFFFFFFu;
struct RingSt {
	// (scalars, never an array indexed at run time: that would go to scratch)
	uint32_t tb0, tb1;       // the tile (first packet) of slot 0 / 1, RING_NONE: free
	uint32_t left0, left1;   // its packets not yet finished
	uint32_t any;            // bit s: a packet of slot s's tile has a side word
	uint32_t next;           // the slot the next tile with deferrals takes
	__device__ __forceinline__ void init()
	{
		tb0 = tb1 = RING_NONE;
		left0 = left1 = any = next = 0;
	}
	__device__ __forceinline__ uint32_t tb(int s) const { return s ? tb1 : tb0; }
	__device__ __forceinline__ uint32_t left(int s) const { return s ? left1 : left0; }
	__device__ __forceinline__ void set(int s, uint32_t t, uint32_t l)
	{
		if (s) {
			tb1 = t;
			left1 = l;
		} else {
			tb0 = t;
			left0 = l;
		}
	}
};
// this wave's slots (addresses recomputed at each use: nothing of them stays
// live across the walker engine, whose registers are at their limit)
__device__ __forceinline__ uint2 *ring_rec(Shared &sh)
{
	return (uint2 *)&sh.lay[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))][0];
}
__device__ __forceinline__ uint32_t *ring_side(Shared &sh)
{
	return &sh.lay[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))][256];
}
static_assert(NSD_LDS_LAYERS * 64 >= 2 * 64 * 2 + 2 * 64, "two tiles of compact records and side words");

// Lanes with fin finished packet i with record r and side word sv (0:
// none): into its tile's slot, or straight to HBM when the tile is not in
// the ring.  Wave-uniform call.
__device__ __forceinline__ void ring_put(Shared &sh, RingSt &rs, bool fin, uint32_t i, uint2 r, uint32_t sv,
					 void *__restrict__ rec, uint32_t *__restrict__ side)
{
	const uint32_t tb = i & ~63u;
	const int sl = !fin ? -1 : tb == rs.tb0 ? 0 : tb == rs.tb1 ? 1 : -1;
	if (sl >= 0) {
		ring_rec(sh)[sl * 64 + (i & 63)] = r;
		ring_side(sh)[sl * 64 + (i & 63)] = sv;
	} else if (fin) {
		__builtin_nontemporal_store(v2u{ r.x, r.y }, (v2u *)rec + i);
		if (sv)
			side[i] = sv;
	}
	rs.left0 -= (uint32_t)__popcll(__ballot(sl == 0));
	rs.left1 -= (uint32_t)__popcll(__ballot(sl == 1));
	rs.any |= (__ballot(sl == 0 && sv != 0) ? 1u : 0u) | (__ballot(sl == 1 && sv != 0) ? 2u : 0u);
}

// Store slot s's tile - the records of its packets (lane k: packet tb + k;
// `held`: still on a walker, not stored) in one wave store, its side words
// in another when any is set - and free the slot.  Wave-uniform call.
__device__ __forceinline__ void ring_store(Shared &sh, RingSt &rs, int s, bool held, void *__restrict__ rec,
					   uint32_t *__restrict__ side, uint32_t n, int lane)
{
	wave_sync_lds();
	const uint32_t i = rs.tb(s) + (uint32_t)lane;
	const bool on = !held && i < n;
	const uint2 r = ring_rec(sh)[s * 64 + lane];
	if (on)
		__builtin_nontemporal_store(v2u{ r.x, r.y }, (v2u *)rec + i);
	if (rs.any & (1u << s)) {
		const uint32_t sv = ring_side(sh)[s * 64 + lane];
		if (on)
			side[i] = sv;
	}
	wave_sync_lds();   // (the slot's next writes after these reads)
	rs.set(s, RING_NONE, 0);
	rs.any &= ~(1u << s);
}

// A tile with `nd` deferred packets (nd > 0) takes the next slot (free:
// ring_turn) with the records of the packets the fast walk finished (`done`)
__device__ __forceinline__ void ring_open(Shared &sh, RingSt &rs, uint32_t base, uint32_t nd, bool done, uint2 r,
					  uint32_t sv, int lane)
{
	const int s = (int)rs.next;
	if (done) {
		ring_rec(sh)[s * 64 + lane] = r;
		ring_side(sh)[s * 64 + lane] = sv;
	}
	rs.set(s, base, nd);
	rs.any |= __ballot(done && sv != 0) ? 1u << s : 0u;
	rs.next ^= 1u;
}

// The LINKTYPE_LINUX_SLL head (dissector_sll.c:39-82): pulls nothing; in
// print_full the next ops come from the packet's sockaddr_ll (sll_next).
template <int MODE>
__device__ __forceinline__ void sll_head(Shared &sh, WalkOut &w, const uint32_t *__restrict__ sll, uint32_t i)
{
	const uint32_t w0 = sll ? sll[5 * (size_t)i] : 0u;       // sll_family | sll_protocol << 16
	const uint32_t w2 = sll ? sll[5 * (size_t)i + 2] : 0u;   // sll_hatype | pkttype << 16 | halen << 24
	const uint32_t hatype = w2 & 0xFFFF;
	const uint32_t proto = __builtin_bswap16((uint16_t)(w0 >> 16));
	w.chain = NSD_OPS_SLL;
	w.n = 1;
	atomicAdd(&sh.ops[NSD_OPS_SLL], 1u);
	w.id = sll_next(hatype, proto, MODE, sh.step[32 + NSD_L2H(proto)]);
}

// A wave's pending list (wq, `wcap` slots: one per packet the wave visits)
// holds the ICMPv4 checksums left to icmp_pass from the front (npend) and
// the host-rendered leaves left to leaf_pass from the back (nleaf); a packet
// ends in at most one of the two.
struct Pending {
	uint64_t *wq;
	uint32_t wcap;
	uint32_t npend, nleaf;
};

// leaf entry: packet index | leaf start << 32 | ops id << 48 (16-byte
// records), packet index | leaf start << 32 | tail << 48 (compact records,
// whose record has no tail; the id is the chain's last)
__device__ __forceinline__ uint64_t leaf_entry(uint32_t i, uint32_t start, int id)
{
	return (uint64_t)i | (uint64_t)(start & 0xFFFF) << 32 | (uint64_t)id << 48;
}
__device__ __forceinline__ uint64_t leaf_entry_c(uint32_t i, uint32_t start, uint32_t tail)
{
	return (uint64_t)i | (uint64_t)(start & 0xFFFF) << 32 | (uint64_t)(tail & 0xFFFF) << 48;
}

// What a lane whose general walk ended leaves behind (wave-uniform call):
// an ICMPv4 message past its windows and a host-rendered leaf go to the
// wave's pending list, an ext chain to the pool (layers 0..5 from the record
// registers, 6..11 from the wave's LDS list, deeper ones already in the
// entry), then the record and the flag counts.  Compact records keep a
// chain of 7..12 layers in the packet's side word (ids 6..11, 5 bits each:
// one coalesced 4-byte store instead of a pool entry, C4 -25 %); only
// longer chains (entry taken at layer 12 by take_deep) write an entry, with
// ids only.
template <int MODE, bool CR, bool RING>
__device__ __forceinline__ void emit_general(Shared &sh, RingSt &rs, bool fin, WalkOut &w, uint32_t i,
					     uint32_t caplen, const GenSink<CR> &g, void *__restrict__ rec, Pending &pq,
					     FlagCnt &fc, int lane)
{
	// a host-rendered leaf's end is walked by the leaf pass: into the 16-byte
	// record's cursor, or (compact records with side words) into the side
	// word of a chain of up to 6 layers or word 2 of an entry past 12 layers
	const bool lf = fin && w.leaf != 0 &&
			(!CR || (g.side && (w.n <= NSD_REC_MAX_LAYERS || (w.ext_on && w.slot != 0xFFFFFFFFu &&
									   w.n <= NSD_EXT_MAX_LAYERS))));
	const uint64_t lm = __ballot(lf);
	if (lf) {
		pq.wq[pq.wcap - 1 - (pq.nleaf + lanes_below(lm))] =
			CR ? leaf_entry_c(i, w.data, w.tail) : leaf_entry(i, w.data, w.leaf);
		if (CR)
			w.flags |= NSD_F_LEAF_END;
	}
	pq.nleaf += (uint32_t)__popcll(lm);
	uint64_t *const wq = pq.wq;
	uint32_t &npend = pq.npend;
	if (MODE == PRINT_NORM) {
		const bool pnd = fin && w.icmp_pend;
		const uint64_t pm = __ballot(pnd);
		if (pnd)
			wq[npend + lanes_below(pm)] = pend_entry(i, w.icmp_off, w.icmp_len);
		npend += (uint32_t)__popcll(pm);
	}
	constexpr uint32_t DEEP = NSD_REC_MAX_LAYERS + NSD_LDS_LAYERS;
	static_assert(DEEP == NSD_CREC_MAX_LAYERS, "side words hold the LDS-listed layers");
	// (a 7..12-layer chain's side word: ids 6..11, never 0)
	const bool sw = CR && fin && w.n > NSD_REC_MAX_LAYERS && !w.ext_on;
	if constexpr (CR) {
		if (sw && g.side && !RING)
			g.side[i] = w.offB;
		if (sw && !g.side)
			w.flags |= NSD_F_OVERFLOW;   // no side words: the pool is smaller than the batch
	}
	const bool ex = fin && (CR ? w.ext_on : w.need_ext);
	if (__ballot(ex)) {
		const bool tk = ex && !w.ext_on;
		if (!CR) {
			const uint32_t sb = ext_take(g, tk, NSD_EXT_WORDS(DEEP));
			if (tk) {
				w.slot = sb;
				w.ext_on = true;
			}
		}
		if (ex && w.slot == 0xFFFFFFFFu)
			w.flags |= NSD_F_OVERFLOW;   // the pool is full
		if (ex && w.slot != 0xFFFFFFFFu) {
			uint32_t *e = g.pool + w.slot;
			const uint32_t nl = w.n < NSD_EXT_MAX_LAYERS ? w.n : NSD_EXT_MAX_LAYERS;
			auto lv = [&](uint32_t j) -> uint32_t {
				if (CR)   // ids only
					return j < NSD_REC_MAX_LAYERS ? (w.chain >> (5 * j)) & 31
								      : (w.offB >> (5 * (j - NSD_REC_MAX_LAYERS))) & 31;
				if (j < NSD_REC_MAX_LAYERS)
					return ((w.chain >> (5 * j)) & 31) | (uint32_t)off_of(w, j) << 16;
				return j < nl ? g.lay[(j - NSD_REC_MAX_LAYERS) * 64 + lane] : 0u;
			};
			// layers 0 .. DEEP-1 (deeper ones are in the entry already)
			static_assert(DEEP % 4 == 0 && DEEP <= 16, "whole uint4 groups of a short entry");
			*(uint4 *)e = make_uint4(i, nl, 0, 0);
#pragma unroll
			for (uint32_t g0 = 0; g0 < DEEP; g0 += 4)
				if (g0 == 0 || nl > g0)
					*(uint4 *)(e + 4 + g0) = make_uint4(lv(g0), lv(g0 + 1), lv(g0 + 2), lv(g0 + 3));
		}
	}
	if (CR && RING)
		ring_put(sh, rs, fin, i, crec_of(w), sw && g.side ? w.offB : 0u, rec, g.side);
	else if (fin)
		put_rec<CR>(rec, i, w);
	fc.add(w, caplen, fin);
}

// The general walk's pool: every lane of a wave is also a walker that holds
// (at most) one packet the fast walk could not finish.  A tile's deferred
// packets are handed to free walkers in lane order; a session stages the
// windows of the walkers that need one (new, or suspended at the end of
// their window) and steps every walker that can step.  While packets are
// still waiting for a walker, a session stops as soon as NSD_REFILL walkers
// are idle, to take them; the tile's last session runs until every walker
// is done or suspended, and the suspended ones are carried to the next
// tile's session (their next window would be restaged anyway).  So a tile
// costs one window wait (1.15 sessions per C4 tile against 2 rounds) and
// its steps run with refilled lanes (7.2 layer steps per C4 tile against 9.8
// when each tile's deferred lanes are walked to their ends).
struct Walker {
	WalkOut w;
	uint64_t d;       // its packet's descriptor
	uint32_t i;       // its packet's index
	uint32_t wb;      // aligned position of its staged window
	uint32_t wl;      // bytes of it staged
	bool have;        // holds a packet
	bool stage;       // its window must be (re)staged before it steps again
};

// The ring at the point where the previous tile's held stores go out
// (walk_tiles, before the next tile's loads): every tile whose packets are
// all finished is stored, and the slot the next tile with deferrals takes,
// if its tile still has packets on walkers (walked across two more tiles),
// stores the finished ones and leaves the ring.
__device__ __forceinline__ void ring_turn(Shared &sh, RingSt &rs, const Walker &wk, void *__restrict__ rec,
					  uint32_t *__restrict__ side, uint32_t n, int lane)
{
#pragma unroll
	for (int k = 0; k < 2; k++)
		if (rs.tb(k) != RING_NONE && rs.left(k) == 0)
			ring_store(sh, rs, k, false, rec, side, n, lane);
	const int s = (int)rs.next;
	if (rs.tb(s) != RING_NONE) {
		// which of the tile's packets walkers hold: a byte per packet in the
		// wave's take() map (free outside take)
		const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
		sh.tmap[wv][lane] = 0;
		wave_sync_lds();
		if (wk.have && (wk.i & ~63u) == rs.tb(s))
			sh.tmap[wv][wk.i & 63] = 1;
		wave_sync_lds();
		const bool held = sh.tmap[wv][lane] != 0;
		ring_store(sh, rs, s, held, rec, side, n, lane);
	}
}

// How much of a walker's window to stage (walkers()).  An HBM read costs
// whole 128-byte lines, and a chain's later layers need only a few bytes
// each (c_step's `need`: 4 for an extension header, none for a leaf), so a
// window that runs into the next line past the chain's end fetches a line
// nothing reads.  The window ends at the end of the line holding the next
// layer's needed bytes, or of the line after it when fewer than
// NSD_WIN_AHEAD bytes of that line would be left past them (the chain then
// likely goes on there); a walker whose next layer needs no bytes (a leaf)
// stages nothing.  C4 (line model over the oracle's layer starts): 1.09
// staged windows per packet against 0.93, 233 against 279 distinct bytes
// per packet.
__device__ __forceinline__ uint32_t window_len(uint64_t abs_wb, uint64_t abs_cur, uint32_t need)
{
	if (!need)
		return 0;
	uint64_t le = ((abs_cur + need - 1) | 127) + 1;
	if (le - (abs_cur + need) < NSD_WIN_AHEAD)
		le += 128;
	const uint64_t l = le - abs_wb;
	return l < WIN2 ? (uint32_t)l : (uint32_t)WIN2;
}

// Hand the waiting packets (lanes with pnd: the tile's deferred packets, walk
// state pw after walk_init / the fast walk's layers) to free walkers: the
// waiting lane of rank r goes to the free walker of rank r (a lane map in
// LDS, then one shuffle per state word).
template <bool CR>
__device__ __forceinline__ void take(Shared &sh, Walker &wk, bool &pnd, const WalkOut &pw, uint32_t pi, uint64_t pd,
				     int lane, int wv);

template <int MODE, bool CR, bool RING>
__device__ __forceinline__ void walkers(Shared &sh, RingSt &rs, const uint8_t *__restrict__ frames, void *__restrict__ rec,
					const GenSink<CR> &g, Pending &pq, FlagCnt &fc, Walker &wk, bool &pnd,
					const WalkOut &pw, uint32_t pi, uint64_t pd, bool drain)
{
	constexpr int ROW = WIN2 / 4;
	const int lane = threadIdx.x & 63;
	const int wv = threadIdx.x >> 6;
	for (;;) {
		take<CR>(sh, wk, pnd, pw, pi, pd, lane, wv);
		if (!__ballot(wk.have))
			break;
		const bool more = __ballot(pnd) != 0;
		// ---- a session
		const uint64_t off = NSD_DESC_OFF(wk.d);
		const uint32_t caplen = NSD_DESC_CAPLEN(wk.d), m = (uint32_t)off & 15;
		const bool st = wk.have && wk.stage;
		const uint64_t fbase = (uint64_t)(frames + (off & ~15ull));
		if (st) {
			wk.wb = (wk.w.data + m) & ~15u;
			wk.wl = window_len(fbase + wk.wb, fbase + wk.w.data + m, sh.step[wk.w.id & 31] >> 25);
		}
		if (__ballot(st)) {
			// (the window's HBM address and extent are recomputed from the
			// descriptor rather than kept live across the walk: registers)
			const uint32_t lim = caplen + m;   // first aligned position past the frame
			uint32_t rem = st && wk.wb < lim ? lim - wk.wb : 0u;
			rem = rem < wk.wl ? rem : wk.wl;
			stage_glds<WIN2>(&sh.win[wv][0], fbase + wk.wb, rem, lane);
		}
		const LSrc<false, WIN2> src{ &sh.win[wv][lane * ROW], sh.lay3, sh.step, frames + off,
					     caplen, m, wk.wb, false, swz_of((uint32_t)lane, WIN2 / 16) << 2, wk.wl };
		bool susp, act;
		uint32_t info;   // the stepping ops' rule word (gen_step reuses it)
		auto ready = [&](uint32_t inf) {
			const bool run = wk.have && wk.w.id != 0;
			info = inf;
			susp = run && src.near_end_i(wk.w.data, info);
			act = run && !susp;
			const uint64_t am = __ballot(act);
			// stop when no walker can step, or enough are idle to take
			// waiting packets
			return am != 0 && !(more && __popcll(am) <= 64 - NSD_REFILL);
		};
		// (a plain leaf - TCP / UDP / ESP / NoNext, no byte read - run in
		// the step that reached it, so its chain ends an iteration earlier:
		// C4 1.002 against 0.956 ms, r06 gpu_s8; every iteration pays the
		// fold's record code)
		auto step = [&]() -> uint32_t {
			gen_step<MODE>(src, act, wk.w, g, info);
			return src.step(wk.w.id);
		};
		if constexpr (CR) {
			// one exit, at the bottom: the exits of a loop that tests at the
			// top merge into one latch, where the compiler copied 13 walk
			// state registers per step (C4 -1.3 %; the 16-byte form's
			// walkers spill this way: 1.73 against 1.70 ms)
			if (ready(src.step(wk.w.id))) {
				do {
				} while (ready(step()));
			}
		} else {
			for (uint32_t inf = src.step(wk.w.id); ready(inf);)
				inf = step();
		}
		wave_sync_lds();
		const bool fin = wk.have && wk.w.id == 0;
		emit_general<MODE, CR, RING>(sh, rs, fin, wk.w, wk.i, caplen, g, rec, pq, fc, lane);
		wk.have = wk.have && !fin;
		wk.stage = susp;
		if (!drain && !more)
			break;   // every walker is done or suspended: the next tile
	}
}

template <bool CR>
__device__ __forceinline__ void take(Shared &sh, Walker &wk, bool &pnd, const WalkOut &pw, uint32_t pi, uint64_t pd,
				     int lane, int wv)
{
	const uint64_t P = __ballot(pnd), F = __ballot(!wk.have);
	if (!P || !F)
		return;
	const uint32_t rp = lanes_below(P), rf = lanes_below(F);
	const uint32_t np = (uint32_t)__popcll(P), nf = (uint32_t)__popcll(F);
	if (pnd && rp < nf)
		sh.tmap[wv][rp] = (uint8_t)lane;
	wave_sync_lds();
	const bool get = !wk.have && rf < np;
	const int src = get ? (int)sh.tmap[wv][rf] : lane;
	const uint32_t x0 = __shfl(pi, src, 64);
	const uint32_t x1 = __shfl((uint32_t)pd, src, 64);
	const uint32_t x2 = __shfl((uint32_t)(pd >> 32), src, 64);
	const uint32_t x3 = __shfl(pw.data | pw.tail << 16, src, 64);
	// (a deferred chain has at most 4 layers: Ethernet, 2 tags, IP)
	const uint32_t x4 = __shfl((uint32_t)pw.ip_csum | (uint32_t)pw.flags << 16 | pw.n << 24 | (uint32_t)pw.id << 27,
				   src, 64);
	const uint32_t x5 = __shfl(pw.chain, src, 64);
	uint32_t x6 = 0, x7 = 0, x8 = 0;
	if (!CR) {
		x6 = __shfl((uint32_t)pw.offA, src, 64);
		x7 = __shfl((uint32_t)(pw.offA >> 32), src, 64);
		x8 = __shfl(pw.offB, src, 64);
	}
	if (get) {
		wk.i = x0;
		wk.d = x1 | (uint64_t)x2 << 32;
		walk_init(wk.w, x3 >> 16, (int)(x4 >> 27));
		wk.w.data = x3 & 0xFFFF;
		wk.w.ip_csum = (uint16_t)x4;
		wk.w.flags = (uint8_t)(x4 >> 16);
		wk.w.n = (x4 >> 24) & 7;
		wk.w.chain = x5;
		if (!CR) {
			wk.w.offA = x6 | (uint64_t)x7 << 32;
			wk.w.offB = x8;
		}
	}
	wk.have = wk.have || get;
	wk.stage = wk.stage || get;
	pnd = pnd && rp >= nf;
}

// plain_walk maps protocols 6 / 17 without the eth_lay3
// lookup fast_walk makes: the table must agree
constexpr uint8_t k_plain_lay3[256] = NSD_LAY3_TABLE;

// ---- pending ICMPv4 checksums -------------------------------------------------
// Runs after both passes (the records are final): the block's waves take its
// lists in 64-entry pieces and patch the flags byte of the records whose sum
// is bad.  Eight lanes per message, 8 messages per wave at a time: lane
// `sub` of a group sums the interior chunks 1 + sub + 8t (whole 16-byte
// loads, no masking; each group instruction reads 128 contiguous bytes, a
// line, where four lanes read half a line per instruction: C3 -1.6 %), U of
// them in flight per lane; sub-lanes 0 and 1 also take the message's first
// and last chunk with the bytes outside the message masked.  A message then
// costs a few wave instructions per KiB instead of one wave per message.
template <int U, bool CR, int L = NSD_CSUM_LANES>
__device__ __forceinline__ void icmp_pass(Shared &sh, const uint8_t *__restrict__ frames,
					  const uint64_t *__restrict__ desc, void *__restrict__ rec,
					  const uint64_t *__restrict__ pend, uint32_t region)
{
	const int lane = threadIdx.x & 63;
	const int wv = threadIdx.x >> 6;
	static_assert(L == 4 || L == 8 || L == 16, "lanes per message");
	const uint32_t sub = lane & (L - 1), grp = lane / L;
	uint32_t bad = 0;
	for (int l = 0; l < WAVES; l++) {
		const uint32_t cnt = sh.pcnt[l];
		const uint64_t *list = pend + ((size_t)blockIdx.x * WAVES + l) * (region / WAVES);
		// the block's waves split each list in 64-entry pieces
		for (uint32_t k0 = 64 * ((wv + l) % WAVES); k0 < cnt; k0 += 64 * WAVES) {
			const bool on = k0 + lane < cnt;
			const uint64_t e = on ? list[k0 + lane] : 0;
			const uint32_t i = (uint32_t)e;
			const uint32_t moff = (uint32_t)(e >> 32) & 0xFFFF, mlen = (uint32_t)(e >> 48);
			const uint64_t a = (on ? NSD_DESC_OFF(desc[i]) : 0) + moff;
			const uint32_t nb = on ? (mlen & ~1u) : 0u;
			for (uint32_t q = 0; q < 64 && k0 + q < cnt; q += 64 / L) {
				const int src = (int)(q + grp);
				const uint32_t alo = __shfl((uint32_t)a, src, 64);
				const uint32_t ahi = __shfl((uint32_t)(a >> 32), src, 64);
				const uint32_t mnb = __shfl(nb, src, 64);
				const bool mon = k0 + (uint32_t)src < cnt;
				const uint32_t s0 = alo & 15, endb = s0 + mnb;
				const uint32_t nch = mon ? (endb + 15) >> 4 : 0u;
				const uint4 *base = (const uint4 *)(frames + ((((uint64_t)ahi << 32) | alo) & ~15ull));
				// edge chunks, masked: chunk 0 on sub-lane 0, chunk nch-1 on sub-lane 1
				uint32_t sum = 0;
				const uint32_t je = sub == 0 ? 0u : nch - 1;
				if ((sub == 0 && nch > 0) || (sub == 1 && nch > 1))
					sum = csum_chunk(base[je], 16 * je, s0, endb);
				// interior chunks [1, nch - 1)
				for (uint32_t j = 1 + sub; __ballot(j + 1 < nch); j += L * U) {
					uint4 v[U];
#pragma unroll
					for (int u = 0; u < U; u++) {
						const uint32_t jj = j + L * u;
						v[u] = jj + 1 < nch ? base[jj] : make_uint4(0, 0, 0, 0);
					}
#pragma unroll
					for (int u = 0; u < U; u++) {
						sum = sum_halves(v[u].x, sum);
						sum = sum_halves(v[u].y, sum);
						sum = sum_halves(v[u].z, sum);
						sum = sum_halves(v[u].w, sum);
					}
				}
				sum = (sum >> 16) + (sum & 0xffff);   // folding keeps the zero test
#pragma unroll
				for (int x = 1; x < L; x <<= 1)
					sum += __shfl_xor(sum, x, 64);
				const uint32_t mi = __shfl(i, src, 64);
				const bool isbad = mon && sub == 0 && csum_final(sum) != 0;
				if (isbad) {
					uint8_t *nf = (uint8_t *)rec + nflags_at<CR>(mi);
					*nf = *nf | NSD_F_ICMP_BAD;
				}
				bad += FlagCnt::pc(isbad);
			}
		}
	}
	if (lane == 0 && bad)
		atomicAdd(&sh.cnt[NSD_CNT_ICMP_BAD], (unsigned long long)bad);
}

// ---- the walk ------------------------------------------------------------------
// Every packet of the block's grid-stride tiles, one wave per 64-packet tile:
// the fast walk over each packet's first 64 bytes, then the general walk's
// walkers take the packets it could not finish (walkers); ICMPv4 messages
// past the windows and host-rendered leaves go to the wave's pending list
// (pq).
// A wave's issue priority (s_setprio) from its progress: level 0 (the first
// quarter of its tiles) issues first, level 3 last.  The SIMD arbiter
// otherwise favours the oldest waves, and a CU's blocks arrive in rounds of
// one block per CU: with 4 blocks per CU the first round finished its tiles
// 20 % ahead of the fourth (C4: 835 against 1031 us; C3: 305 against 422),
// whose waves then ran the launch's tail with the CU a quarter full.
// (Priority by round alone only swapped which round lagged.)  Since the
// group tiles balance a CU's blocks, it still gives C3 0.7 % but costs
// walker-heavy batches 1 % (C4): the launcher turns it off for those
// (`prio`, from the schedule sample).
__device__ __forceinline__ void prio_level(uint32_t lvl)
{
	if (lvl == 0)
		__builtin_amdgcn_s_setprio(3);
	else if (lvl == 1)
		__builtin_amdgcn_s_setprio(2);
	else if (lvl == 2)
		__builtin_amdgcn_s_setprio(1);
	else
		__builtin_amdgcn_s_setprio(0);
}

template <int MODE, bool CR, bool RING>
__device__ __forceinline__ void walk_tiles(Shared &sh, const uint8_t *__restrict__ frames,
					   const uint64_t *__restrict__ desc, uint32_t n, int start_id,
					   void *__restrict__ rec, uint32_t *__restrict__ ext, uint32_t ext_words,
					   uint32_t *__restrict__ ext_used, uint32_t chunk,
					   const uint32_t *__restrict__ sll, Pending &pq,
					   unsigned long long *__restrict__ sched, uint32_t *__restrict__ gtiles,
					   uint32_t prio)
{
	constexpr int ROW = row_of(WIN1);
	auto &s_win = sh.win;
	unsigned long long *const s_cnt = sh.cnt;
	const uint8_t *const s_lay3 = sh.lay3;
	const int lane = threadIdx.x & 63;
	const int wv = threadIdx.x >> 6;

	const uint32_t stride = gridDim.x * BLOCK;
	uint64_t *const wq = pq.wq;
	// compact records: pool words [0, n) are the packets' side words, entries
	// come after (a pool of fewer than n words has neither: an entry never
	// lies where a consumer looks for a side word)
	const bool side = CR && ext_words >= n;
	const GenSink<CR> g{ ext, ext_words, ext_used, chunk, &sh.wc[wv][0], sh.ops, &sh.lay[wv][0],
			 CR ? n : 0u, side ? ext : nullptr };
	FlagCnt fc;
	uint32_t ndefer = 0;
	uint32_t base = blockIdx.x * BLOCK + wv * 64;   // this wave's tile; whole waves iterate

	if (MODE != PRINT_NORM && MODE != PRINT_LESS) {
		// every process() is NULL: no chain (dissector.c:51-53)
		for (; base < n; base += stride) {
			const uint32_t i = base + lane;
			fc.pkts += FlagCnt::pc(i < n);
			if (i < n) {
				const uint32_t caplen = NSD_DESC_CAPLEN(desc[i]);
				if constexpr (CR)
					__builtin_nontemporal_store(v2u{ 0u, 0u }, (v2u *)rec + i);
				else
					store_rec((uint4 *)rec, i, make_uint4(0, caplen << 16, 0, 0));
				fc.bytes += caplen;
			}
		}
		fc.flush(s_cnt, lane);
		return;
	}

	// Tiles of a CU group.  A launch of 4 blocks per CU places blocks b,
	// b + G, b + 2G, b + 3G (G = grid / 4) on one CU, and the SIMD arbiter
	// runs the first-placed block's waves ahead of the later ones (C4: the
	// rounds ended their tiles at 835 / 881 / 945 / 1031 us).  So the group's
	// 16 waves share its grid-stride tiles: the group's j-th tile is row
	// j / 16 of the grid stride, block b + ((j / 4) % 4) G, wave j % 4 (the
	// static order, so the waves still sweep the batch front to back, and
	// tile numbers grow with j), and a wave takes the next j from the
	// group's counter (a line of its own in the workspace, zeroed before
	// each launch by zero_tiles; one counter for the whole grid serialised
	// its atomics: 2.3x slower).
	// The atomic for tile t+2 is issued a tile ahead and its return read then
	// (hipcc's atomic optimizer would wait for it at once: the offset it
	// cannot prove uniform).  A wave asks only while its pending list has
	// room for an entry from every packet of the tiles it holds, the new one
	// and its walkers: the lists hold twice a wave's even share plus four
	// tiles (fused_region), so a group's waves cannot all stop for room
	// while its tiles are left.  Grids that are not 4 blocks per CU share
	// per block.  Compact records only (the 16-byte form's walk state leaves
	// no registers for it: 12 VGPRs spilled).
	constexpr bool DYN = CR;
	const uint32_t ntiles = (n + 63) / 64;
	const uint32_t nw = gridDim.x * WAVES;
	const bool grp4 = gridDim.x % NSD_GROUP_BLOCKS == 0;
	const uint32_t G = grp4 ? gridDim.x / NSD_GROUP_BLOCKS : gridDim.x, R = grp4 ? NSD_GROUP_BLOCKS : 1u;
	const uint32_t grp = blockIdx.x % G;
	uint32_t *const gctr = gtiles + LINE_WORDS * grp;
	auto tile_of = [&](uint32_t j) -> uint32_t {   // the group's j-th tile's first packet (n: none)
		const uint32_t k = j / (4 * R), r = (j / 4) % R, w = j % 4;
		const uint64_t t = (uint64_t)k * nw + (grp + r * G) * 4 + w;
		return t < ntiles ? (uint32_t)t * 64 : n;
	};
	uint32_t gv = 0;
	bool asked = false;
	auto ask = [&](uint32_t held) {
		const uint32_t used = pq.npend + pq.nleaf;
		asked = used + 64u * (held + 2) <= pq.wcap;
		if (asked && lane == 0) {
			uint32_t z;
			asm volatile("v_mov_b32 %0, 0" : "=v"(z));
			gv = atomicAdd(gctr + z, 1u);
		}
	};
	auto take = [&]() -> uint32_t {   // the asked tile (n: none)
		if (!asked)
			return n;
		asked = false;
		return tile_of((uint32_t)__builtin_amdgcn_readfirstlane((int)gv));
	};
	uint32_t nb1 = n, nb2 = n;
	if constexpr (DYN) {
		ask(0);
		base = take();
		if (base < n) {
			ask(1);
			nb1 = take();
			if (nb1 < n)
				ask(2);   // for tile t+2, read when tile t is walked
		}
	} else {
		nb1 = base + stride < n ? base + stride : n;
	}
	// software pipeline: tile t walked while tile t+1's chunks and tile t+2's
	// descriptors are in flight
	if (base >= n)
		return;
	uint64_t d0 = (base + lane < n) ? desc[base + lane] : 0;
	uint64_t d1 = (nb1 < n && nb1 + lane < n) ? desc[nb1 + lane] : 0;
	Chunks<WIN1> ch;
	stage_load<WIN1>(ch, frames, d0, lane);
	Walker wk;
	walk_init(wk.w, 0, 0);
	wk.d = 0;
	wk.i = 0;
	wk.wb = 0;
	wk.wl = 0;
	wk.have = false;
	wk.stage = false;

	// late: the next tile's chunks load after this tile's walkers (this tile's
	// predecessor was walker-heavy, below)
	bool late = false;
	HeldSt<CR> hs;   // the previous tile's record / pending-list stores
	hs.ri = hs.pp = 0xFFFFFFFFu;
	// compact records: the wave's record ring (RecRing), slot rs for the
	// next tile
	constexpr bool RG = CR && RING;
	RingSt rs;
	rs.init();
	// (one more pass after the last tile drains the walkers: the engine is
	// inlined once)
	// this wave's even share of tiles and the ones walked, for prio_level
	const uint32_t share = (ntiles + nw - 1) / nw;
	uint32_t done = 0, lvl = 0xFFu;
	for (;;) {
		if (CR && prio) {   // (the 16-byte form's walk state leaves no registers for it)
			const uint32_t l = done < share ? 4u * done / share : 3u;
			if (l != lvl) {
				lvl = l;
				prio_level(l);
			}
			done++;
		}
		const bool last = base >= n;
		const uint32_t i = base + lane;
		const bool valid = i < n;
		const uint64_t off = NSD_DESC_OFF(d0);
		const uint32_t caplen = NSD_DESC_CAPLEN(d0);
		WalkOut w;
		walk_init(w, caplen, valid ? start_id : 0);
		bool deferred = false;
		uint64_t d2 = 0;
		if (!last) {
			stage_write(&s_win[wv][0], ch, lane);
			hs.flush(rec, wq);   // tile t-1's stores, before tile t+1's loads
			if (RG)
				ring_turn(sh, rs, wk, rec, g.side, n, lane);
			// prefetch: descriptors of tile t+2, chunks of tile t+1
			if constexpr (DYN) {
				nb2 = take();
				if (nb2 < n)
					ask(3);   // tiles t .. t+2 held
			}
			const uint32_t b2 = DYN ? nb2 : base + 2 * stride;
			d2 = (b2 < n && b2 + lane < n) ? desc[b2 + lane] : 0;
			const uint32_t b1 = DYN ? nb1 : base + stride;
			if (b1 < n && !late)
				stage_load<WIN1>(ch, frames, d1, lane);
			wave_sync_lds();

			uint32_t fw = FW_DONE;
			const LSrc<true, WIN1> src{ &s_win[wv][lane * ROW], s_lay3, nullptr, frames + off, caplen,
						    (uint32_t)off & 15, 0, false };
			if (valid)
				fw = fast_walk<MODE, false, true>(src, caplen, w);
			deferred = fw != FW_DONE;
			ndefer += FlagCnt::pc(deferred);
			wave_sync_lds();
			const bool done = valid && !deferred;
			if (MODE == PRINT_NORM) {
				// ICMPv4 messages past the window: listed for the checksum pass, which
				// patches the record if the sum is bad
				const bool pnd = w.icmp_pend && done;
				const uint64_t pmask = __ballot(pnd);
				hs.hold_pend(wq, pend_entry(i, w.icmp_off, w.icmp_len),
					     pnd ? pq.npend + lanes_below(pmask) : 0xFFFFFFFFu);
				pq.npend += (uint32_t)__popcll(pmask);
			}
			// per-ops counts from the finished chains, grouped by chain word
			// (ids are >= 1, so equal chain words imply equal layer counts) for
			// the first two distinct chains of the tile (C2: one), the rest per
			// lane (C3: -4.5 % against looping over every distinct chain)
			{
				uint32_t key = done ? w.chain : 0xFFFFFFFFu;
				for (int it = 0;; it++) {
					const uint64_t pm = __ballot(key != 0xFFFFFFFFu);
					if (!pm)
						break;
					if (it == 2) {
						// more than two distinct chains in the tile: the rest
						// count their own layers (the LDS serialises them)
						if (key != 0xFFFFFFFFu)
							for (uint32_t k = 0; k < w.n; k++)
								atomicAdd(&sh.ops[(key >> (5 * k)) & 31], 1u);
						break;
					}
					const int leader = __ffsll((unsigned long long)pm) - 1;
					const uint32_t lk = __shfl(key, leader, 64);
					const uint64_t m = __ballot(key == lk);
					if (lane == leader) {
						const uint32_t cnt = (uint32_t)__popcll(m);
						for (uint32_t k = 0, nl = w.n; k < nl; k++)
							atomicAdd(&sh.ops[(lk >> (5 * k)) & 31], cnt);
					}
					if (key == lk)
						key = 0xFFFFFFFFu;
				}
			}
			// a leaf the fast walk finished (ARP, DCCP): its end in the side word
			const bool lend = CR && g.side && done && (w.flags & NSD_F_HOST);
			if (lend)
				w.flags |= NSD_F_LEAF_END;
			const uint32_t nd = (uint32_t)__popcll(__ballot(deferred));
			if (RG && nd) {
				ring_open(sh, rs, base, nd, done, crec_of(w), lend ? w.data : 0u, lane);
			} else if (CR && !RG) {
				if (lend)
					g.side[i] = w.data;
				hs.hold_rec(i, crec_of(w), done);
			} else {
				if (lend)
					g.side[i] = w.data;
				if (done)
					put_rec<CR>(rec, i, w);
			}
			fc.add(w, caplen, done);
			// the deferred packets' walk state for the general walk: from the
			// start (FW_RESTART: other link types, MPLS, deeper tag stacks, bytes
			// past the first window) or from where the fast walk stopped
			// (FW_RESUME: its layers recorded; its finished chains are counted by
			// chain word, these are counted here)
			if (deferred) {
				if (fw == FW_RESTART) {
					walk_init(w, caplen, start_id);
					if (start_id == NSD_OPS_SLL)
						sll_head<MODE>(sh, w, sll, i);
				} else {
					for (uint32_t k = 0; k < w.n; k++)
						atomicAdd(&sh.ops[(w.chain >> (5 * k)) & 31], 1u);
				}
			}
		}
		// (the walkers carried over are suspended: their windows are
		// restaged anyway, so this tile's staging may reuse their rows)
		bool pnd = deferred;
		const bool many = __popcll(__ballot(pnd)) >= NSD_L2PF;
		if (__ballot(pnd || wk.have)) {
			// (the walkers wait for their windows anyway: the held stores go
			// first, and nothing is held across the engine's registers)
			hs.flush(rec, wq);
			walkers<MODE, CR, RG>(sh, rs, frames, rec, g, pq, fc, wk, pnd, w, i, d0, last);
		}
		if (last) {
			hs.flush(rec, wq);
			if (RG)
				ring_turn(sh, rs, wk, rec, g.side, n, lane);   // every walker is done: the ring's last tiles
			break;
		}
		// After a walker-heavy tile (C4) the next tile's chunks load here, with
		// L2-allocating loads, rather than a tile ahead: its walkers' first
		// windows then find the packets' first lines in L2 (loaded a tile
		// ahead, those lines had left L2 by the time the walkers staged them:
		// C4 400 -> 349 B/packet, 1.152 -> 1.107 ms on one box).  The chunk
		// registers are dead during the walkers either way.
		if (late && (DYN ? nb1 : base + stride) < n)
			stage_load<WIN1, false, false>(ch, frames, d1, lane);
		late = many;
		d0 = d1;
		d1 = d2;
		if constexpr (DYN) {
			base = nb1;
			nb1 = nb2;
			nb2 = n;
		} else {
			base += stride;
		}
	}
	if (CR && prio)
		__builtin_amdgcn_s_setprio(0);   // the leaf and checksum passes at the neutral level
	fc.flush(s_cnt, lane);
	// the pending list held every entry (ask()'s room rule: a packet adds at
	// most one, ICMPv4 from the front or leaf from the back, and the lists
	// hold two shares plus four tiles); a broken invariant overwrote the next
	// wave's list: counted, and the counters then differ from any oracle's
	if (lane == 0 && pq.npend + pq.nleaf > pq.wcap)
		atomicAdd(&s_cnt[NSD_CNT_LISTOVF], 1ull);
	// the schedule sample (a launch the launcher samples passes its pair)
	if (sched && lane == 0 && ndefer)
		atomicAdd(&sched[0], (unsigned long long)ndefer);
	if (sched && lane == 0 && pq.npend)
		atomicAdd(&sched[1], (unsigned long long)pq.npend);
}

// ---- host-rendered leaves -------------------------------------------------------
// The leaves the wave's general walk ended in (ARP / LLDP / IGMP / DCCP /
// ICMPv6 130-154; ARP and DCCP inside the fast window finish in fast_walk):
// one lane per entry walks the leaf parser's pulls over the frame in HBM
// (nsd_leaf.h) and rewrites the record's cursor word.  A pass of its own,
// after the tiles, so the LLDP TLV and ND-option loops do not add to the
// walk's register peak.  The wave reads back only what it wrote itself.
template <int MODE, bool CR>
__device__ __forceinline__ void leaf_pass(const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc,
					  void *__restrict__ rec, uint32_t *__restrict__ pool, const Pending &pq)
{
	if (!pq.nleaf)
		return;
	__threadfence();   // the wave's record and list stores complete before its loads below
	for (uint32_t k = threadIdx.x & 63; k < pq.nleaf; k += 64) {
		const uint64_t e = pq.wq[pq.wcap - 1 - k];
		const uint32_t i = (uint32_t)e, start = (uint32_t)(e >> 32) & 0xFFFF;
		const uint64_t d = desc[i];
		const HbmBytes src{ frames + NSD_DESC_OFF(d), NSD_DESC_CAPLEN(d) };
		if constexpr (!CR) {
			const int id = (int)(e >> 48);
			uint32_t *const y = (uint32_t *)((uint4 *)rec + i) + 1;   // data_off | tail_off << 16
			const uint32_t tail = __hip_atomic_load(y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 16;
			*y = leaf_end<MODE>(src, id, start, tail) | tail << 16;
		} else {
			// the leaf is the chain's last layer: its id from the record (inline
			// ids) or the entry (ids only); its end into the side word or entry
			const uint32_t tail = (uint32_t)(e >> 48);
			const uint64_t rv = __hip_atomic_load((uint64_t *)rec + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const uint2 r = make_uint2((uint32_t)rv, (uint32_t)(rv >> 32));
			const uint32_t nf = (r.y >> 16) & 0xFF, n = nf & 7;
			uint32_t *loc;
			int id;
			if (n != NSD_N_EXT) {
				id = (int)((r.x >> (5 * (n - 1))) & 31);
				loc = pool + i;
			} else {
				const uint32_t nl = __hip_atomic_load(pool + r.x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xFFFF;
				id = (int)(__hip_atomic_load(pool + r.x + NSD_EXT_HDR_WORDS + nl - 1, __ATOMIC_RELAXED,
							     __HIP_MEMORY_SCOPE_AGENT) & 31);
				loc = pool + r.x + 2;
			}
			*loc = leaf_end<MODE>(src, id, start, tail);
		}
	}
}

// One launch per batch.  Each block of the persistent grid walks its
// grid-stride tiles (fast walk + continuations), walks the leaves its waves
// left pending, then sums the ICMPv4 messages they left pending; a later
// phase reads only what the same block wrote (its pending lists), so the
// phases need a block barrier, not a grid-wide one.
// the fused launch's group tile counters (walk_tiles): word 0 of each
// 128-byte line.  A kernel rather than hipMemsetAsync: with the memset
// captured into a HIP graph the counters held garbage from the second
// replay on (tools/dbg_graph.py), so no tile was walked.
__global__ void zero_tiles(uint32_t *__restrict__ gtiles, uint32_t groups)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < groups)
		gtiles[LINE_WORDS * i] = 0;
}

template <int MODE, bool CR, bool RING = false>
__global__ __launch_bounds__(BLOCK, NSD_MINW) void dissect_all(
	const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc, uint32_t n, int start_id,
	void *__restrict__ rec, uint32_t *__restrict__ ext, uint32_t ext_words,
	uint32_t *__restrict__ ext_used, uint32_t chunk, unsigned long long *__restrict__ counters,
	uint64_t *__restrict__ pend, uint32_t region, const uint32_t *__restrict__ sll,
	unsigned long long *__restrict__ sched, uint32_t *__restrict__ gtiles, uint32_t prio)
{
	__shared__ Shared sh;
	if (threadIdx.x < 64)
		sh.step[threadIdx.x] = threadIdx.x < 32 ? c_step[threadIdx.x] : c_lay2h.e[threadIdx.x - 32];
	if (threadIdx.x < 32)
		sh.ops[threadIdx.x] = 0;
	if (threadIdx.x < 2 * WAVES)
		sh.wc[threadIdx.x >> 1][threadIdx.x & 1] = 0;
	block_init(sh.cnt, sh.lay3);   // (its barrier orders the stores above too)

	// this wave's pending list (a wave visits region / WAVES packets)
	Pending pq{ pend + ((size_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * (region / WAVES), region / WAVES, 0,
		    0 };
	walk_tiles<MODE, CR, RING>(sh, frames, desc, n, start_id, rec, ext, ext_words, ext_used, chunk, sll, pq,
				   sched, gtiles, prio);
	if (MODE == PRINT_NORM || MODE == PRINT_LESS)
		leaf_pass<MODE, CR>(frames, desc, rec, ext, pq);
	if ((threadIdx.x & 63) == 0)
		sh.pcnt[threadIdx.x >> 6] = pq.npend;
	if (MODE == PRINT_NORM) {
		__syncthreads();   // records final, pending lists and counts complete
		icmp_pass<NSD_CSUM_U, CR>(sh, frames, desc, rec, pend, region);
	}
	block_flush(sh.cnt, counters);
	if (threadIdx.x < 32 && sh.ops[threadIdx.x])
		atomicAdd(&counters[NSD_CNT_OPS + threadIdx.x], (unsigned long long)sh.ops[threadIdx.x]);
}

} // namespace nsd

#endif
