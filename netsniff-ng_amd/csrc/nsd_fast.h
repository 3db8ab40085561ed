// nsd_fast.h - the split kernel (dissect_fast): the fast walk of every tile,
// then each wave's list through the fused kernel's walker pool.
#ifndef NSD_FAST_H
#define NSD_FAST_H

#include "nsd_fused.h"

namespace nsd {

// ==== the split schedule ===========================================================
// One launch per batch, as the fused schedule.  dissect_fast first runs the
// fast walk of every tile with two tiles' chunks in flight per wave (3
// resident blocks per CU, NSD_FAST_BPC; the loop's registers and LDS are
// only what the fast walk needs), writes the records of the packets it
// finishes, sums the ICMPv4 messages they leave pending and appends every
// packet it cannot finish to its wave's deferral list.  A block whose waves
// deferred packets then walks them itself: each wave runs the walker pool
// (walkers(), the general walk) over its own list (walk_lists), in the same
// LDS words as the fast rows.  The fused kernel's tile loop carries the
// walker pool's registers through every tile, which C2 and C3 - nearly
// nothing deferred - paid for in latency hiding.
//
// A fast wave's list (`cap` slots of 32 bytes):
//   deferrals from the front: { packet, data | tail << 16,
//     ip_csum | flags << 16 | n << 24 | id << 27, chain },
//     { descriptor, starts of layers 1..4 (a byte each: the fast window) }
//   pending ICMPv4 checksums from the back: { packet, off | len << 16,
//     the message's words before off, summed and weighted like the pass
//     (below) }, { descriptor }
// The descriptor rides along so the tail and the checksum pass read no
// desc[] (and the tail knows the next chunk's window addresses early).

constexpr int FROW = WIN1 / 4;   // fast rows: 16 dwords, 16-byte slots XOR-swizzled by swz_of(q, 4)

struct FastShared {
	alignas(16) uint32_t win[WAVES][64 * FROW];   // fast rows
	unsigned long long cnt[NSD_NCOUNTERS];        // block counters
	uint32_t ops[32];                             // block per-ops layer counts
	uint8_t lay3[256];                            // eth_lay3
	uint32_t pcnt[WAVES];                         // pending checksums per wave
};

// stage_write into the split schedule's rows: chunk c of packet q at slot
// c ^ swz(q) of its 16-dword row (ds_write_b128; the 8 lanes of a store
// group cover two whole rows: no bank conflict)
__device__ __forceinline__ void stage_write_sw(uint32_t *wwin, const Chunks<WIN1> &ch, int lane)
{
#pragma unroll
	for (int r = 0; r < 4; r++) {
		const int t = r * 64 + lane;
		const int q = t / 4, c = t % 4;
		const uint32_t nv = (ch.nv >> (8 * r)) & 0xFF;
		uint32_t w[4] = { ch.v[r].x, ch.v[r].y, ch.v[r].z, ch.v[r].w };
		if (nv < 16) {
#pragma unroll
			for (int j = 0; j < 4; j++) {
				const uint32_t bp = 4 * j;
				if (bp >= nv)
					w[j] = 0;
				else if (bp + 4 > nv)
					w[j] &= (1u << ((nv - bp) * 8)) - 1u;
			}
		}
		*(uint4 *)(wwin + q * FROW + ((c ^ swz_of((uint32_t)q, 4)) << 2)) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

// a folded 16-bit partial sum in the pass's byte weighting: the pass sums a
// message's bytes as aligned little-endian halves, which weights them by 256
// (mod 0xFFFF) against the reference's words when the message starts at an
// odd address (see the ICMPv4 checksum helpers above); so is the partial
__device__ __forceinline__ uint32_t fold_weighted(uint32_t sum, bool odd)
{
	sum = (sum >> 16) + (sum & 0xFFFF);
	sum = (sum >> 16) + (sum & 0xFFFF);
	return odd ? ((sum & 0xFF) << 8 | sum >> 8) : sum;
}

// The plain IPv4 chain (PRINT_NORM, split schedule): Ethernet (type 0x0800,
// no tag), IPv4 without options (first byte 0x45), then TCP or UDP, in a
// frame of at least 42 bytes.  For such a packet fast_walk (nsd_walk.h) reads
// bytes 12..33 and nothing past them, all inside the window, and ends with
// the chain Ethernet, IPv4, TCP / UDP at offsets 0 / 14 / 34 (proto_ethernet.c,
// proto_ipv4.c:34-204 incl. the total-length trim, proto_tcp.c / proto_udp.c).
// plain_is tells from bytes 12..23 whether the packet is one; plain_walk
// then reads bytes 12..35 (7 row dwords, byte funnel shifts) and gives
// fast_walk's result from them alone (re-read rather than kept: registers).
// A tile takes this path only when every valid lane's packet is plain
// (wave-uniform), so a mixed tile runs fast_walk alone.
// plain_is / plain_walk map protocol 6 / 17 to TCP / UDP without the eth_lay3
// lookup fast_walk makes: the table must agree
static_assert(k_plain_lay3[6] == NSD_OPS_TCP && k_plain_lay3[17] == NSD_OPS_UDP,
	      "plain_walk's protocol map differs from eth_lay3");

__device__ __forceinline__ bool plain_is(const LSrc<true, WIN1> &s, uint32_t caplen)
{
	const uint32_t r = s.m + 12, j = r >> 2, sh = r & 3;
	const uint32_t d12 = __builtin_amdgcn_alignbyte(s.dw(j + 1), s.dw(j), sh);
	const uint32_t d20 = __builtin_amdgcn_alignbyte(s.dw(j + 3), s.dw(j + 2), sh);
	const uint32_t proto = d20 >> 24;
	return caplen >= 42 && (d12 & 0xFFFFFFu) == 0x450008u && (proto == 6 || proto == 17);
}

__device__ __forceinline__ void plain_walk(const LSrc<true, WIN1> &s, uint32_t caplen, WalkOut &w)
{
	const uint32_t r = s.m + 12, j = r >> 2, sh = r & 3;   // j + 6 <= 12: inside the 16-dword row
	const uint32_t w0 = s.dw(j), w1 = s.dw(j + 1), w2 = s.dw(j + 2), w3 = s.dw(j + 3), w4 = s.dw(j + 4),
		       w5 = s.dw(j + 5), w6 = s.dw(j + 6);
	const uint32_t d12 = __builtin_amdgcn_alignbyte(w1, w0, sh), d16 = __builtin_amdgcn_alignbyte(w2, w1, sh),
		       d20 = __builtin_amdgcn_alignbyte(w3, w2, sh), d24 = __builtin_amdgcn_alignbyte(w4, w3, sh),
		       d28 = __builtin_amdgcn_alignbyte(w5, w4, sh), d32 = __builtin_amdgcn_alignbyte(w6, w5, sh);
	// calc_csum over the 10 header words at 14..32 (csum.h:12-27)
	uint32_t sum = (d12 >> 16) + (d32 & 0xFFFF);
	sum = __builtin_amdgcn_sad_u16(d16, 0u, sum);
	sum = __builtin_amdgcn_sad_u16(d20, 0u, sum);
	sum = __builtin_amdgcn_sad_u16(d24, 0u, sum);
	sum = __builtin_amdgcn_sad_u16(d28, 0u, sum);
	sum = (sum >> 16) + (sum & 0xffff);
	sum += sum >> 16;
	w.ip_csum = (uint16_t)~sum;
	// the total-length trim (ihl 5: no options)
	const int32_t x = (int32_t)__builtin_bswap16((uint16_t)d16) - 20;
	if (x >= 0 && (uint32_t)x < caplen - 34)
		w.tail = 34 + (uint32_t)x;
	const bool tcp = (d20 >> 24) == 6;
	const int l4 = tcp ? NSD_OPS_TCP : NSD_OPS_UDP;
	w.chain = NSD_OPS_ETHERNET | NSD_OPS_IPV4 << 5 | (uint32_t)l4 << 10;
	w.offA = (uint64_t)14 << 16 | (uint64_t)34 << 32;
	w.n = 3;
	const uint32_t len = w.tail - 34, hl = tcp ? 20u : 8u;
	w.data = len >= hl ? 34 + hl : 34;
}

// The fast loop's tiles: a static front and a shared tail.  Wave gw of nw walks
// tiles gw, gw + nw, ... below `tail0` exactly as a grid stride would (no
// atomics, the batch swept front to back).  The tiles from tail0 on - the
// last rounds of the grid stride - are handed out at run time, because the
// waves do not end together (C2: the XCDs' waves end between 172 and 188 us
// on average, and a launch lasts until the last).  A ticket is a pair of
// adjacent tiles: head h of `nheads` hands out pairs h, h + nheads, ... of
// the tail in ascending order, one returning atomic of lane 0 per ticket on
// the head's own 128-byte line.  A block's home head is blockIdx.x % nheads
// (blocks with equal blockIdx.x % 8 share an XCD, and nheads is a multiple
// of 8 when there are 8 or more, so a head's pullers sit on one XCD).  A
// wave whose head has run out moves on to the next head (the next XCD's),
// NSD_TAIL_TRIES times at most, and stays there; it does not visit them all.
// A ticket is asked when the one before is read, two tiles before its first
// descriptor is due (ask / take, as walk_tiles: an atomic's answer takes 1 -
// 3 us under streaming load, a tile 1.6; asked one tile ahead, C2 kept 1.5 %
// of the 2.2).  The launcher makes the
// front's rounds even.  The loop's control state is declared wave-uniform
// (`uni`): hipcc takes threadIdx.x >> 6 for divergent, and then kept tile
// numbers, list counts and the ticket's head and flags in vector registers,
// which cost dissect_fast<PRINT_NORM, true> its last ones (2 spilled).
// Room: a packet adds at most one entry to the wave's list (a deferral from
// the front or an ICMPv4 remainder from the back), and a wave asks only while
// the list has room for every packet of the five tiles it holds and the new
// two; once it may not ask, or its heads are empty, it asks no more, so no
// tile follows a missing one in its pipeline.  Liveness: a wave stopped for
// room walks at least cap / 64 - 1 tiles, i.e. rounds + rounds / 5 - 1 (the
// launcher's cap), which is rounds + 2 or more (rounds >= NSD_TAIL_MIN_ROUNDS
// = 16); a head's home waves alone then hold more than the head's tiles (4
// blocks a head or more), so while a head has tiles left one of its home
// waves can still ask.  heads == nullptr: every tile is static.
template <int MODE, bool CR>
__device__ __forceinline__ void fast_tiles(FastShared &sh, const uint8_t *__restrict__ frames,
					   const uint64_t *__restrict__ desc, uint32_t n, int start_id,
					   void *__restrict__ rec, const uint32_t *__restrict__ sll, uint32_t *__restrict__ side,
					   uint4 *__restrict__ list, uint32_t cap, uint32_t &ndef, uint32_t &nicmp,
					   uint32_t *__restrict__ heads, uint32_t tail0, uint32_t nheads)
{
	const int lane = threadIdx.x & 63;
	// (wave-uniform, and said so: hipcc takes threadIdx.x >> 6 for divergent and
	// then keeps the loop's whole control state - tile numbers, list counts, the
	// ticket's head and flags - in vector registers)
	const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	const uint32_t stride = gridDim.x * BLOCK;
	FlagCnt fc;
	auto uni = [](uint32_t x) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
	uint32_t base = uni(blockIdx.x * BLOCK + wv * 64);

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
		fc.flush(sh.cnt, lane);
		return;
	}
	if (base >= n)
		return;
	uint32_t *const rows = &sh.win[wv][0];
	// Descriptors are loaded unconditionally, from a clamped index (a load
	// under a branch leaves hipcc unsure whether it is pending, and it then
	// waits vmcnt(0) for the chunks, i.e. for every load in flight); a lane
	// past the batch keeps the last packet's descriptor: it only stages that
	// frame's window, it walks nothing (valid is false) and counts nothing.
	auto dsc = [&](uint32_t b) -> uint64_t {
		return desc[b < n && b + lane < n ? b + lane : n - 1];
	};
	// One tile at `base` whose chunks are in `ch` (descriptors d0): write them
	// to the rows, reuse `ch` for the chunks of the tile two strides on
	// (descriptors dpre), walk the tile.
	auto tile = [&](Chunks<WIN1> &ch, const uint64_t d0, const uint64_t dpre) {
		const uint32_t i = base + lane;
		const bool valid = i < n;
		const uint64_t off = NSD_DESC_OFF(d0);
		const uint32_t caplen = NSD_DESC_CAPLEN(d0);
		WalkOut w;
		walk_init(w, caplen, valid ? start_id : 0);
		stage_write_sw(rows, ch, lane);
		// (issued past the batch's last tile too, from the clamped
		// descriptor - loads skipped on some paths also make hipcc wait
		// vmcnt(0))
		stage_load<WIN1, true>(ch, frames, dpre, lane);
		wave_sync_lds();
		uint32_t fw = FW_DONE;
		const LSrc<true, WIN1> src{ rows + lane * FROW, sh.lay3, nullptr, frames + off, caplen,
					    (uint32_t)off & 15, 0, false, swz_of((uint32_t)lane, 4) << 2 };
		// (every lane's row is staged, a lane past the batch from the clamped descriptor)
		const bool plain = MODE == PRINT_NORM && start_id == NSD_OPS_ETHERNET &&
				   __ballot(valid && !plain_is(src, caplen)) == 0;
		if (plain) {
			if (valid)
				plain_walk(src, caplen, w);
		} else if (valid) {
			fw = fast_walk<MODE, true>(src, caplen, w);
		}
		const bool deferred = fw != FW_DONE;
		wave_sync_lds();
		const bool done = valid && !deferred;
		if (plain) {
			// a plain tile (Ethernet / IPv4 / TCP or UDP, every packet done, no
			// ICMPv4, no leaf, no deferral): its counts straight from three
			// ballots - packets, bad IPv4 sums, trims - and the TCP share
			const uint64_t vm = __ballot(valid), tm = __ballot(valid && w.chain >> 10 == NSD_OPS_TCP);
			const uint32_t nv = (uint32_t)__popcll(vm), nt = (uint32_t)__popcll(tm);
			if (lane == 0) {
				atomicAdd(&sh.ops[NSD_OPS_ETHERNET], nv);
				atomicAdd(&sh.ops[NSD_OPS_IPV4], nv);
				if (nt)
					atomicAdd(&sh.ops[NSD_OPS_TCP], nt);
				if (nv - nt)
					atomicAdd(&sh.ops[NSD_OPS_UDP], nv - nt);
			}
			if (valid)
				put_rec_st<CR>(rec, i, w);
			fc.pkts += nv;
			fc.ipbad += FlagCnt::pc(valid && w.ip_csum != 0);
			fc.trim += FlagCnt::pc(valid && w.tail < caplen);
			if (valid)
				fc.bytes += caplen;
			return;
		}
		if (MODE == PRINT_NORM) {
			// ICMPv4 messages past the window, from the back of the list
			const bool pnd = w.icmp_pend && done;
			const uint64_t pm = __ballot(pnd);
			if (pnd) {
				const uint32_t part = fold_weighted(w.icmp_sum, ((uint32_t)off + w.icmp_off) & 1);
				uint4 *e = list + (size_t)(cap - 1 - (nicmp + lanes_below(pm))) * SW;
				st_b128(e, make_uint4(i, w.icmp_off | w.icmp_len << 16, part, 0));
				st_b128(e + 1, make_uint4((uint32_t)d0, (uint32_t)(d0 >> 32), 0, 0));
			}
			nicmp = uni(nicmp + (uint32_t)__popcll(pm));
		}
		// per-ops counts of the finished chains, grouped by chain word (as
		// walk_tiles)
		{
			uint32_t key = done ? w.chain : 0xFFFFFFFFu;
			for (int it = 0;; it++) {
				const uint64_t pm = __ballot(key != 0xFFFFFFFFu);
				if (!pm)
					break;
				if (it == 2) {
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
		if (CR && side && done && (w.flags & NSD_F_HOST)) {
			// a leaf the fast walk finished (ARP, DCCP): its end in the side word
			st_b32(side + i, w.data);
			w.flags |= NSD_F_LEAF_END;
		}
		if (done)
			put_rec_st<CR>(rec, i, w);
		fc.add(w, caplen, done);
		// the deferred packets' walk state, for walk_lists: from the start
		// (FW_RESTART; the SLL head is run here) or where the fast walk stopped
		// (FW_RESUME: its layers are counted here)
		const uint64_t dm = __ballot(deferred);
		if (dm) {
			if (deferred) {
				if (fw == FW_RESTART) {
					walk_init(w, caplen, start_id);
					if (start_id == NSD_OPS_SLL) {
						const uint32_t w0 = sll ? sll[5 * (size_t)i] : 0u;
						const uint32_t w2 = sll ? sll[5 * (size_t)i + 2] : 0u;
						const uint32_t proto = __builtin_bswap16((uint16_t)(w0 >> 16));
						w.chain = NSD_OPS_SLL;
						w.n = 1;
						atomicAdd(&sh.ops[NSD_OPS_SLL], 1u);
						w.id = sll_next(w2 & 0xFFFF, proto, MODE, c_lay2h.e[NSD_L2H(proto)]);
					}
				} else {
					for (uint32_t k = 0; k < w.n; k++)
						atomicAdd(&sh.ops[(w.chain >> (5 * k)) & 31], 1u);
				}
				// (n < 8 and id < 32: a deferred chain holds at most the SLL
				// head, Ethernet, 2 tags and IP, layer 0 at 0 and the others
				// inside the 64-byte window)
				uint4 *e = list + (size_t)(ndef + lanes_below(dm)) * SW;
				st_b128(e, make_uint4(i, w.data | w.tail << 16,
						      (uint32_t)w.ip_csum | (uint32_t)w.flags << 16 | w.n << 24 |
							      (uint32_t)w.id << 27,
						      w.chain));
				const uint32_t offs = CR ? 0u
							 : ((uint32_t)(w.offA >> 16) & 0xFF) | ((uint32_t)(w.offA >> 32) & 0xFF) << 8 |
								   ((uint32_t)(w.offA >> 48) & 0xFF) << 16 | (w.offB & 0xFF) << 24;
				st_b128(e + 1, make_uint4((uint32_t)d0, (uint32_t)(d0 >> 32), offs, 0));
			}
			ndef = uni(ndef + (uint32_t)__popcll(dm));
		}
	};
	// two tiles' chunks in flight while one is walked: two register sets that
	// swap roles (the loop unrolled by two), descriptors three tiles ahead
	// The wave's tiles in order: `base`, then b1 and b2 (n: none), then what
	// step() gives - the static front's next tile, `nxt`, while it lies below
	// `slim`, a ticket's after that.  (The launcher shares the tail only when
	// the front has more than three rounds: base, b1 and b2 are static, and
	// the first ticket is asked when the front's last tile is fetched.)
	const uint32_t ntiles = (n + 63) / 64;
	const uint32_t slim = heads ? tail0 * 64 : n;
	uint32_t cur = heads ? blockIdx.x % nheads : 0, tries = nheads > 1 ? 0 : NSD_TAIL_TRIES;
	bool more = heads != nullptr, asked = false;
	uint32_t gv = 0;
	auto draw = [&]() {
		if (lane == 0) {
			uint32_t z;
			asm volatile("v_mov_b32 %0, 0" : "=v"(z));   // (keeps hipcc's atomic optimizer off: walk_tiles)
			gv = atomicAdd(heads + LINE_WORDS * cur + z, 1u);
		}
	};
	auto ask = [&]() {
		asked = more && ndef + nicmp + 64u * 7 <= cap;
		more = asked;
		if (asked)
			draw();
	};
	uint32_t second = n;   // the other tile of the last ticket (n: none, or taken)
	auto take = [&]() -> uint32_t {   // the asked ticket's first tile (n: none)
		if (!asked)
			return n;
		asked = false;
		// the ticket's first tile (32 bits do: a head counts from zero in every
		// launch and gives fewer tickets than the batch has tiles plus one per
		// wave that finds it empty; a tile is walked only when it is below ntiles)
		auto tile_of = [&]() -> uint32_t {
			const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)gv);
			return tail0 + 2 * (cur + k * nheads);
		};
		// (the ticket asked two tiles ago is read here, outside the loop below:
		// its wait counts the loads issued since and leaves them in flight)
		uint32_t t = tile_of();
		// this head is empty: on to the next one, at once (the wave is about to
		// run dry; the room for the tiles is reserved already).  Nested tests,
		// not a loop: hipcc folds a loop's ticket read into the one above and
		// then waits for every load in flight at each ticket.
		auto next = [&]() {
			tries++;
			cur = cur + 1 == nheads ? 0 : cur + 1;
			draw();
			t = tile_of();
		};
		static_assert(NSD_TAIL_TRIES == 3, "take(): one nested test per try");
		if (t >= ntiles && tries < NSD_TAIL_TRIES) {
			next();
			if (t >= ntiles && tries < NSD_TAIL_TRIES) {
				next();
				if (t >= ntiles && tries < NSD_TAIL_TRIES)
					next();
			}
		}
		if (t >= ntiles) {
			more = false;
			return n;
		}
		// (the batch's last tile without a partner: no tile may follow the
		// missing one in the pipeline, so the wave asks no more)
		second = t + 1 < ntiles ? (t + 1) * 64 : n;
		if (second == n)
			more = false;
		return t * 64;
	};
	uint32_t nxt = uni(base + 3 * stride);
	// (a ticket is asked when the one before is read, two tiles before its
	// first descriptor is due: an atomic's answer takes 1 - 3 us under
	// streaming load, a tile 1.6)
	auto step = [&]() -> uint32_t {
		uint32_t b;
		if (nxt < slim) {
			b = nxt;
			nxt = uni(nxt + stride);
			if (nxt >= slim)
				ask();
		} else if (second < n) {
			b = second;
			second = n;
		} else {
			b = take();
			ask();
		}
		return b;
	};
	uint32_t b1 = base + stride < slim ? base + stride : n, b2 = base + 2 * stride < slim ? base + 2 * stride : n;
	uint64_t d0 = dsc(base), d1 = dsc(b1), d2 = dsc(b2);
	Chunks<WIN1> chA, chB;
	stage_load<WIN1, true>(chA, frames, d0, lane);
	stage_load<WIN1, true>(chB, frames, d1, lane);
	for (;;) {
		uint32_t b3 = uni(step());
		uint64_t d3 = dsc(b3);
		tile(chA, d0, d2);
		d0 = d1;
		d1 = d2;
		d2 = d3;
		base = uni(b1);
		b1 = b2;
		b2 = b3;
		if (base >= n)
			break;
		b3 = uni(step());
		d3 = dsc(b3);
		tile(chB, d0, d2);
		d0 = d1;
		d1 = d2;
		d2 = d3;
		base = uni(b1);
		b1 = b2;
		b2 = b3;
		if (base >= n)
			break;
	}
	drain_stores();   // the loop's records, list entries and side words are complete (and its last ticket has come)
	// the list held every entry (ask()'s room rule); a broken invariant
	// overwrote the next wave's list: counted, as walk_tiles does
	if (lane == 0 && ndef + nicmp > cap)
		atomicAdd(&sh.cnt[NSD_CNT_LISTOVF], 1ull);
	fc.flush(sh.cnt, lane);
}

// The fast kernel's pending ICMPv4 checksums (fast_tiles' list backs): as
// icmp_pass, four lanes per message; the remainder [off, off + len) is summed
// from HBM and the partial sum of the words before it added.
template <int U, bool CR>
__device__ __forceinline__ void fast_icmp_pass(FastShared &sh, const uint8_t *__restrict__ frames,
					       const uint64_t *__restrict__ desc, void *__restrict__ rec,
					       const uint4 *__restrict__ lists, uint32_t cap)
{
	const int lane = threadIdx.x & 63;
	const int wv = threadIdx.x >> 6;
	const uint32_t sub = lane & 3, grp = lane >> 2;
	uint32_t bad = 0;
	for (int l = 0; l < WAVES; l++) {
		const uint32_t cnt = sh.pcnt[l];
		const uint4 *list = lists + ((size_t)blockIdx.x * WAVES + l) * cap * SW;
		for (uint32_t k0 = 64 * ((wv + l) % WAVES); k0 < cnt; k0 += 64 * WAVES) {
			const bool on = k0 + lane < cnt;
			const uint4 *ep = list + (size_t)(cap - 1 - (k0 + lane)) * SW;
			const uint4 e = on ? ep[0] : make_uint4(0, 0, 0, 0);
			const uint32_t i = e.x;
			const uint64_t a = (on ? NSD_DESC_OFF((uint64_t)ep[1].y << 32 | ep[1].x) : 0) + (e.y & 0xFFFF);
			const uint32_t nb = e.y >> 16;
			for (uint32_t q = 0; q < 64 && k0 + q < cnt; q += 16) {
				const int src = (int)(q + grp);
				const uint32_t alo = __shfl((uint32_t)a, src, 64);
				const uint32_t ahi = __shfl((uint32_t)(a >> 32), src, 64);
				const uint32_t mnb = __shfl(nb, src, 64);
				const uint32_t part = __shfl(e.z, src, 64);
				const bool mon = k0 + (uint32_t)src < cnt;
				const uint32_t s0 = alo & 15, endb = s0 + mnb;
				const uint32_t nch = mon ? (endb + 15) >> 4 : 0u;
				const uint4 *base = (const uint4 *)(frames + ((((uint64_t)ahi << 32) | alo) & ~15ull));
				uint32_t sum = sub == 0 ? part : 0u;
				const uint32_t je = sub == 0 ? 0u : nch - 1;
				if ((sub == 0 && nch > 0) || (sub == 1 && nch > 1))
					sum += csum_chunk(base[je], 16 * je, s0, endb);
				for (uint32_t j = 1 + sub; __ballot(j + 1 < nch); j += 4 * U) {
					uint4 v[U];
#pragma unroll
					for (int u = 0; u < U; u++) {
						const uint32_t jj = j + 4 * u;
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
				sum = (sum >> 16) + (sum & 0xffff);
				sum += __shfl_xor(sum, 1, 64);
				sum += __shfl_xor(sum, 2, 64);
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

// The split schedule's tail: each wave hands the deferrals of its own fast
// loop (`list`, `cnt` entries from the front) to its walker pool
// (walkers()), 64 of them (a chunk) at a time; then, as the fused kernel,
// the block walks the leaves and sums the ICMPv4 checksums its walks left
// pending (the waves' own lists at `pend`, `region` / WAVES slots per wave).
// Chunk entries are loaded two chunks ahead, and while chunk c's walkers
// run, the first windows of chunk c + 1 (at each packet's cursor) are
// touched into L2 by 4-byte LDS-DMA loads (no VGPR waits for them): its
// sessions then stage from L2.  s_touch: the touches' LDS-DMA target (never
// read).  Block-uniform call: the pool's set-up and passes have barriers.
template <int MODE, bool CR>
__device__ __forceinline__ void walk_lists(Shared &sh, uint32_t *s_touch, const uint8_t *__restrict__ frames,
					   const uint64_t *__restrict__ desc, uint32_t n, void *__restrict__ rec,
					   uint32_t *__restrict__ ext, uint32_t ext_words, uint32_t *__restrict__ ext_used,
					   uint32_t chunk, unsigned long long *__restrict__ counters,
					   const uint4 *__restrict__ list, uint32_t cnt, uint64_t *__restrict__ pend,
					   uint32_t region)
{
	if (threadIdx.x < 64)
		sh.step[threadIdx.x] = threadIdx.x < 32 ? c_step[threadIdx.x] : c_lay2h.e[threadIdx.x - 32];
	if (threadIdx.x < 32)
		sh.ops[threadIdx.x] = 0;
	if (threadIdx.x < 2 * WAVES)
		sh.wc[threadIdx.x >> 1][threadIdx.x & 1] = 0;
	block_init(sh.cnt, sh.lay3);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint32_t gw = blockIdx.x * WAVES + wv;
	Pending pq{ pend + (size_t)gw * (region / WAVES), region / WAVES, 0, 0 };
	const bool side = CR && ext_words >= n;
	const GenSink<CR> g{ ext, ext_words, ext_used, chunk, &sh.wc[wv][0], sh.ops, &sh.lay[wv][0],
			     CR ? n : 0u, side ? ext : nullptr };   // (entries past the side words: walk_tiles)
	FlagCnt fc;
	Walker wk;
	walk_init(wk.w, 0, 0);
	wk.d = 0;
	wk.i = 0;
	wk.wb = 0;
	wk.wl = 0;
	wk.have = false;
	wk.stage = false;
	WalkOut pw;
	walk_init(pw, 0, 0);
	RingSt rs;   // (unused: the tail stores its records at once)
	rs.init();

	// the chunk at entry k0 (wave-uniform): lanes past the list's count load nothing
	auto load = [&](uint32_t k0, uint4 &x0, uint4 &x1) {
		x0 = x1 = make_uint4(0, 0, 0, 0);
		if (k0 + lane < cnt) {
			const uint4 *e = list + (size_t)(k0 + lane) * SW;
			x0 = e[0];
			x1 = e[1];
		}
	};
	uint4 c0, c1, n0, n1;
	load(0, c0, c1);
	load(64, n0, n1);
	for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
		{
			// the next chunk's first windows into L2: [cursor, +WIN2) in aligned
			// coordinates, one or two 128-byte lines
			const uint64_t d = (uint64_t)n1.y << 32 | n1.x;
			const uint32_t m = (uint32_t)NSD_DESC_OFF(d) & 15, caplen = NSD_DESC_CAPLEN(d);
			const uint32_t wb = ((n0.y & 0xFFFF) + m) & ~15u;
			const bool on = k0 + 64 + lane < cnt && wb < caplen + m;
			const uint64_t a = (uint64_t)frames + (NSD_DESC_OFF(d) & ~15ull) + wb;
			const bool two = on && (a & 127) != 0 && wb + (128 - (uint32_t)(a & 127)) < caplen + m;
			if (on)
				__builtin_amdgcn_global_load_lds((const void *)(a & ~127ull),
								 (__attribute__((address_space(3))) void *)s_touch, 4, 0, 0);
			if (two)
				__builtin_amdgcn_global_load_lds((const void *)((a & ~127ull) + 128),
								 (__attribute__((address_space(3))) void *)s_touch, 4, 0, 0);
		}
		uint4 m0, m1;
		load(k0 + 128, m0, m1);
		bool pnd = k0 + lane < cnt;
		const uint32_t pi = c0.x;
		const uint64_t pd = (uint64_t)c1.y << 32 | c1.x;
		walk_init(pw, c0.y >> 16, (int)(c0.z >> 27));
		pw.data = c0.y & 0xFFFF;
		pw.ip_csum = (uint16_t)c0.z;
		pw.flags = (uint8_t)(c0.z >> 16);
		pw.n = (c0.z >> 24) & 7;
		pw.chain = c0.w;
		if (!CR) {
			// layer starts 1..4 (layer 0 at 0)
			pw.offA = (uint64_t)(c1.z & 0xFF) << 16 | (uint64_t)((c1.z >> 8) & 0xFF) << 32 |
				  (uint64_t)((c1.z >> 16) & 0xFF) << 48;
			pw.offB = c1.z >> 24;
		}
		walkers<MODE, CR, false>(sh, rs, frames, rec, g, pq, fc, wk, pnd, pw, pi, pd, false);
		c0 = n0;
		c1 = n1;
		n0 = m0;
		n1 = m1;
	}
	{
		bool none = false;
		if (__ballot(wk.have))
			walkers<MODE, CR, false>(sh, rs, frames, rec, g, pq, fc, wk, none, pw, 0, 0, true);
	}
	fc.flush(sh.cnt, lane);
	leaf_pass<MODE, CR>(frames, desc, rec, ext, pq);
	if (lane == 0)
		sh.pcnt[wv] = pq.npend;
	if (MODE == PRINT_NORM) {
		__syncthreads();
		icmp_pass<NSD_CSUM_U, CR>(sh, frames, desc, rec, pend, region);
	}
	block_flush(sh.cnt, counters);
	if (threadIdx.x < 32 && sh.ops[threadIdx.x])
		atomicAdd(&counters[NSD_CNT_OPS + threadIdx.x], (unsigned long long)sh.ops[threadIdx.x]);
}

// The split schedule's kernel.  A block whose waves deferred packets walks
// them itself after its tiles (walk_lists, each wave over its own list, the
// walker pool's LDS in the same words as the fast rows), so a batch the
// fast walk finishes costs no second launch (C2: a walker kernel's empty
// launch cost 4.9 us of 205, at any grid).
template <int MODE, bool CR>
__global__ __launch_bounds__(BLOCK, CR ? NSD_FAST_MINW : NSD_FAST_MINW_FULL) void dissect_fast(
	const uint8_t *__restrict__ frames, const uint64_t *__restrict__ desc, uint32_t n, int start_id,
	void *__restrict__ rec, unsigned long long *__restrict__ counters, uint4 *__restrict__ lists, uint32_t cap,
	const uint32_t *__restrict__ sll, uint32_t *__restrict__ side, unsigned long long *__restrict__ sched,
	uint32_t *__restrict__ ext, uint32_t ext_words, uint32_t *__restrict__ ext_used, uint32_t chunk,
	uint64_t *__restrict__ pend, uint32_t region, uint32_t *__restrict__ heads, uint32_t tail0, uint32_t nheads)
{
	union FastLds {
		FastShared f;
		Shared w;
	};
	__shared__ FastLds su;
	FastShared &sh = su.f;
	if (threadIdx.x < 32)
		sh.ops[threadIdx.x] = 0;
	block_init(sh.cnt, sh.lay3);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const uint32_t gw = blockIdx.x * WAVES + wv;
	uint4 *const list = lists + (size_t)gw * cap * SW;   // this wave's
	uint32_t ndef = 0, nicmp = 0;
	fast_tiles<MODE, CR>(sh, frames, desc, n, start_id, rec, sll, side, list, cap, ndef, nicmp, heads, tail0, nheads);
	if (lane == 0) {
		sh.pcnt[wv] = nicmp;
		if (sched && ndef)
			atomicAdd(&sched[0], (unsigned long long)ndef);
		if (sched && nicmp)
			atomicAdd(&sched[1], (unsigned long long)nicmp);
	}
	if (MODE == PRINT_NORM) {
		__syncthreads();   // records final, the block's pending lists and counts complete
		fast_icmp_pass<NSD_FAST_CSUM_U, CR>(sh, frames, desc, rec, lists, cap);
	}
	block_flush(sh.cnt, counters);
	if (threadIdx.x < 32 && sh.ops[threadIdx.x])
		atomicAdd(&counters[NSD_CNT_OPS + threadIdx.x], (unsigned long long)sh.ops[threadIdx.x]);
	if constexpr (MODE == PRINT_NORM || MODE == PRINT_LESS) {
		// (the barrier also orders the flush's LDS reads before the walker
		// pool's set-up in the same words)
		const bool tail = __syncthreads_or(ndef != 0);
		// The shared tail's heads belong to the library's counter set of this
		// stream (tail_set) and are zero between launches: every block counts
		// itself in the word after the heads once its waves have drawn their
		// last ticket (the barrier above; fast_tiles waited for every ticket it
		// asked; a block without a tile counts too), and the block that comes
		// last zeroes the heads and that word.  Launches on one stream are
		// ordered, so the next one finds zeros.
		if (heads && threadIdx.x == 0 && atomicAdd(heads + LINE_WORDS * nheads, 1u) == gridDim.x - 1) {
			for (uint32_t h = 0; h <= nheads; h++)
				atomicExch(heads + LINE_WORDS * h, 0u);
		}
		if (tail) {
			__shared__ uint32_t s_touch[64];
			walk_lists<MODE, CR>(su.w, s_touch, frames, desc, n, rec, ext, ext_words, ext_used, chunk, counters,
					     list, min(ndef, cap), pend, region);
		}
	}
}

} // namespace nsd

#endif
