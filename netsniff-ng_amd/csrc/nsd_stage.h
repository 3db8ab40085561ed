// nsd_stage.h - device helpers both kernels share (nsd_kernels.hip): window
// sources over LDS, staging, checksum helpers, record stores, the blocks'
// counters, the pending-list entry.
#ifndef NSD_STAGE_H
#define NSD_STAGE_H

#include "nsd_launch.h"
#include "nsd_walk.h"

namespace nsd {

constexpr int WIN1 = 64;         // bytes per staged window, pass 1
constexpr int WIN2 = NSD_WIN2;   // bytes per staged window, general-walk continuation
// fast-walk window row stride in dwords (16-byte aligned rows, see top)
constexpr int row_of(int W) { return W / 4 + 4; }

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
// a chunk in global memory: an address rebuilt from shuffled integers is a
// generic pointer, which compiles to flat_load; flat loads count in lgkmcnt
// too, so every LDS wait of the walk would also wait for the next tile's
// chunks.  Loads through this type are global_load.
typedef __attribute__((address_space(1))) const v4u gv4u;
__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

// The frame's bytes straight from HBM (zero past caplen), for the leaf walks
struct HbmBytes {
	const uint8_t *p;
	uint32_t caplen;
	__device__ __forceinline__ uint8_t b(uint32_t o) const { return o < caplen ? p[o] : 0; }
	__device__ __forceinline__ uint16_t be16(uint32_t o) const { return (uint16_t)(b(o) << 8 | b(o + 1)); }
};

// Byte source over an LDS window (aligned coordinates, see top).
// FAST (the fast walk): the window is a zero-padded row (bytes past caplen
// zeroed by stage_write; 20-dword rows, or the split schedule's 16-dword rows
// with their 16-byte slots XOR-swizzled by sw); bytes outside it are not fetched, the
// source records the miss and the walk gives the packet up to the general
// walk.  Otherwise (the general walk's continuation windows, stage_glds): a
// row of up to WIN bytes filled by LDS-DMA with its 16-byte slots
// XOR-swizzled (dword j at j ^ sw) and nothing zeroed, so every read masks
// the bytes at offsets >= caplen itself; only its first wl bytes are staged
// (a walker's window ends at a line boundary, walkers()), and bytes outside
// them come from HBM.
template <bool FAST, int WIN>
struct LSrc {
	const uint32_t *win;     // this lane's window row
	const uint8_t *lay3t;    // LDS copy of eth_lay3
	const uint32_t *stept;   // LDS copy of c_step, then c_lay2h (general walk)
	const uint8_t *p;        // frame in HBM
	uint32_t caplen;
	uint32_t m;              // off & 15
	uint32_t wb;             // aligned position of window byte 0 (multiple of 16)
	mutable bool miss;
	uint32_t sw;             // continuation rows: slot swizzle (dword index xor)
	uint32_t wl = WIN;       // bytes of the row staged from wb (continuation rows; FAST: WIN)

	__device__ __forceinline__ uint32_t dw(uint32_t j) const { return win[j ^ sw]; }
	__device__ __forceinline__ int lay3(uint32_t key) const { return lay3t[key & 255]; }
	__device__ __forceinline__ uint32_t step(int id) const { return stept[id & 31]; }
	__device__ __forceinline__ uint32_t l2h(uint32_t h) const { return stept[32 + (h & 31)]; }
	// bytes o .. o+3 (little-endian) from the window row: two dwords and a
	// byte funnel shift.  Meaningful only for bytes inside the window (a
	// near_end() budget covers them).  FAST: zero at offsets >= caplen.  The
	// continuation rows are not zeroed past caplen and this read does not
	// mask them: it serves gen_step's layer bytes (B0, the next-ops key) only,
	// every use of which is gated by the layer's first pull succeeding
	// (pulled: the bytes it reads lie before tail <= caplen), so a byte past
	// the frame never reaches a result (C4 -1.4 %: 6 VALU per read).
	__device__ __forceinline__ uint32_t dword_at(uint32_t o) const
	{
		const uint32_t r = o + m - wb;
		uint32_t j = r >> 2;
		j = j > WIN / 4 - 1 ? WIN / 4 - 1 : j;
		const uint32_t v = __builtin_amdgcn_alignbyte(dw(j + 1), dw(j), r & 3);
		if constexpr (FAST)
			return o >= caplen ? 0u : v;
		return v;
	}
	__device__ __forceinline__ bool missed() const { return miss; }
	__device__ __forceinline__ uint8_t b(uint32_t o) const
	{
		const uint32_t r = o + m - wb;
		if constexpr (FAST) {
			if (r < WIN)
				return (uint8_t)(dw(r >> 2) >> ((r & 3) * 8));
			if (o < caplen)
				miss = true;
			return 0;
		} else {
			if (o >= caplen)
				return 0;
			return r < wl ? (uint8_t)(dw(r >> 2) >> ((r & 3) * 8)) : p[o];
		}
	}
	__device__ __forceinline__ uint16_t le16(uint32_t o) const
	{
		const uint32_t r = o + m - wb;
		if (r + 1 < wl && (r & 3) != 3 && (FAST || o + 2 <= caplen))
			return (uint16_t)(dw(r >> 2) >> ((r & 3) * 8));
		return (uint16_t)(b(o) | b(o + 1) << 8);
	}
	__device__ __forceinline__ uint16_t be16(uint32_t o) const
	{
		return (uint16_t)__builtin_bswap16(le16(o));
	}
	// bytes o .. o+15 as four little-endian dwords (5 window dwords + byte
	// funnel shifts).  Only the bytes the caller's near_end() budget covers
	// are meaningful (later ones may come from the next window row); bytes
	// at offsets >= caplen are zero.
	__device__ __forceinline__ void bytes16(uint32_t o, uint32_t &B0, uint32_t &B1, uint32_t &B2,
						uint32_t &B3) const
	{
		const uint32_t r = o + m - wb;
		uint32_t j = r >> 2;
		j = j > WIN / 4 - 1 ? WIN / 4 - 1 : j;
		const uint32_t sh = r & 3;
		const uint32_t w0 = dw(j), w1 = dw(j + 1), w2 = dw(j + 2), w3 = dw(j + 3), w4 = dw(j + 4);
		const bool z = o >= caplen;
		B0 = z ? 0u : __builtin_amdgcn_alignbyte(w1, w0, sh);
		B1 = z ? 0u : __builtin_amdgcn_alignbyte(w2, w1, sh);
		B2 = z ? 0u : __builtin_amdgcn_alignbyte(w3, w2, sh);
		B3 = z ? 0u : __builtin_amdgcn_alignbyte(w4, w3, sh);
	}
	__device__ __forceinline__ bool in_window(uint32_t o, uint32_t nbytes) const
	{
		const uint32_t r = o + m - wb;
		return r < wl && r + nbytes <= wl;
	}
	// window bytes from frame offset o to the window's end
	__device__ __forceinline__ uint32_t window_bytes(uint32_t o) const
	{
		const uint32_t r = o + m - wb;
		return r < wl ? wl - r : 0u;
	}
	// the next layer would read past the staged window (the bytes its parse
	// inspects from its start, c_step's `need`): general walk only
	__device__ __forceinline__ bool near_end(uint32_t o, int id) const
	{
		return near_end_i(o, step(id));
	}
	// the same from the ops' rule word
	__device__ __forceinline__ bool near_end_i(uint32_t o, uint32_t info) const
	{
		const uint32_t need = info >> 25;
		return need && o < caplen && o + m + need > wb + wl;
	}
	// sum of `nwords` little-endian u16 words from `o` (csum.h:16-17)
	__device__ __forceinline__ uint32_t sum16(uint32_t o, uint32_t nwords) const
	{
		uint32_t sum = 0;
		const uint32_t r = o + m - wb;
		if (FAST && !(r & 1)) {
			// the fast walk sums only inside the window (its callers check
			// in_window).  Even start: a leading half, whole dwords four
			// reads at a time (independent LDS reads, one wait per four:
			// an IPv4 header of 20 bytes is one round), a trailing half.
			// Reads past the count are selected away (they stay in LDS).
			uint32_t j = r >> 2, k = nwords;
			if ((r & 2) && k) { sum += dw(j) >> 16; j++; k--; }
			const uint32_t nd = k >> 1;
			for (uint32_t t = 0; t < nd; t += 4) {
				const uint32_t v0 = dw(j + t), v1 = dw(j + t + 1), v2 = dw(j + t + 2), v3 = dw(j + t + 3);
				sum = __builtin_amdgcn_sad_u16(v0, 0u, sum);
				sum = __builtin_amdgcn_sad_u16(t + 1 < nd ? v1 : 0u, 0u, sum);
				sum = __builtin_amdgcn_sad_u16(t + 2 < nd ? v2 : 0u, 0u, sum);
				sum = __builtin_amdgcn_sad_u16(t + 3 < nd ? v3 : 0u, 0u, sum);
			}
			if (k & 1) sum += dw(j + nd) & 0xFFFF;
			return sum;
		}
		if (FAST) {
			// odd start (frames at odd offsets): the dword at window position
			// r, funnel-shifted out of two row dwords, holds the words at o
			// and o + 2; two per round, then a trailing word
			const uint32_t j = r >> 2, sh = r & 3, nd = nwords >> 1;
			for (uint32_t t = 0; t < nd; t += 2) {
				const uint32_t v0 = dw(j + t), v1 = dw(j + t + 1), v2 = dw(j + t + 2);
				sum = __builtin_amdgcn_sad_u16(__builtin_amdgcn_alignbyte(v1, v0, sh), 0u, sum);
				sum = __builtin_amdgcn_sad_u16(t + 1 < nd ? __builtin_amdgcn_alignbyte(v2, v1, sh) : 0u, 0u,
							       sum);
			}
			if (nwords & 1)
				sum += __builtin_amdgcn_alignbyte(dw(j + nd + 1), dw(j + nd), sh) & 0xFFFF;
			return sum;
		}
		if (!(r & 1) && in_window(o, 2 * nwords) && o + 2 * nwords <= caplen) {
			uint32_t j = r >> 2, k = nwords;
			if ((r & 2) && k) { sum += dw(j) >> 16; j++; k--; }
			for (; k >= 2; k -= 2, j++)
				sum = __builtin_amdgcn_sad_u16(dw(j), 0u, sum);   // + both 16-bit halves
			if (k) sum += dw(j) & 0xFFFF;
			return sum;
		}
		for (uint32_t i = 0; i < nwords; i++)
			sum += le16(o + 2 * i);
		return sum;
	}
};

// ---- staging ---------------------------------------------------------------
// Chunk r of the wave: lane (q * CPP + c) % 64 in round (q * CPP + c) / 64
// loads chunk c of packet q's window, so the CPP chunks of one packet are
// read by consecutive lanes as one contiguous, 16-byte aligned segment.

template <int WIN>
struct Chunks {
	static constexpr int CPP = WIN / 16;   // 16-byte chunks per window
	static_assert(CPP <= 4 && WIN <= 255, "a chunk's valid count per byte of nv");
	uint4 v[CPP];
	uint32_t nv;   // valid bytes of chunk r (0..16) in byte r
};

// issue the loads (no wait): in round r, lane (q * CPP + c) % 64 loads chunk
// c of packet q's window = aligned bytes [A_q + 16c, +16), skipped when the
// chunk lies wholly past caplen.  Each lane prepares its own packet's
// aligned start address and frame end once; two shuffles per round hand
// them to the loading lanes (the end, capped at 255 - the window is shorter
// - rides in the address's high dword, a 48-bit VA leaves its top byte
// free).  The count of valid bytes per chunk is kept for stage_write.
// ALL (the split fast loop): every chunk load is issued, chunks wholly past
// caplen too (stage_write zeroes them; a 64-byte window always lies inside
// the frame buffer's NSD_FRAME_PAD): a load under a branch leaves hipcc
// unsure whether it is pending, and it then waits vmcnt(0) for the chunks.
// NT: streaming loads; false where the general walk re-reads the lines soon.
template <int WIN, bool ALL = false, bool NT = true>
__device__ __forceinline__ void stage_load(Chunks<WIN> &ch, const uint8_t *frames, uint64_t my_desc, int lane)
{
	constexpr int CPP = Chunks<WIN>::CPP;
	const uint64_t a = (uint64_t)frames + (NSD_DESC_OFF(my_desc) & ~15ull);
	const uint32_t lim = (uint32_t)NSD_DESC_CAPLEN(my_desc) + ((uint32_t)my_desc & 15);
	const uint32_t hr = (uint32_t)(a >> 32) | (lim < 255u ? lim : 255u) << 24;
	ch.nv = 0;
#pragma unroll
	for (int r = 0; r < CPP; r++) {
		const int t = r * 64 + lane;
		const int q = t / CPP, c = t % CPP;
		const uint32_t alo = __shfl((uint32_t)a, q, 64), ahr = __shfl(hr, q, 64);
		const uint32_t pos = 16u * c, qlim = ahr >> 24;
		const uint32_t nv = qlim > pos ? min(qlim - pos, 16u) : 0u;
		if (ALL || nv) {
			// streaming loads (nt): C2 -9 %, C3 -2 %; C4 +5 % (its general
			// walk re-reads the first line from HBM rather than L2)
			const uint64_t src = ((uint64_t)(ahr & 0xFFFFFFu) << 32 | alo) + pos;
			v4u t4;
			if constexpr (NT)
				t4 = __builtin_nontemporal_load((const gv4u *)src);
			else
				t4 = *(const gv4u *)src;
			ch.v[r] = make_uint4(t4.x, t4.y, t4.z, t4.w);
		} else {
			ch.v[r] = make_uint4(0, 0, 0, 0);
		}
		ch.nv |= nv << (8 * r);
	}
}

// write the chunks to the window rows (row q, dwords 4c..4c+3), zeroing the
// bytes at frame offsets >= caplen
template <int WIN>
__device__ __forceinline__ void stage_write(uint32_t *wwin, const Chunks<WIN> &ch, int lane)
{
	constexpr int CPP = Chunks<WIN>::CPP, ROW = row_of(WIN);
#pragma unroll
	for (int r = 0; r < CPP; r++) {
		const int t = r * 64 + lane;
		const int q = t / CPP, c = t % CPP;
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
		*(uint4 *)(wwin + q * ROW + c * 4) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

// The continuation windows (WIN bytes per lane, CPP = WIN / 16 slots) by
// LDS-DMA: wave-instruction r's lane l fills slot l % CPP of row
// q = r * (64 / CPP) + l / CPP (the destination is lane-linear), loading
// chunk (l % CPP) ^ swz(q) of packet q's window, so row q holds its chunk c
// in slot c ^ swz(q) and the lanes reading one window offset spread over
// the banks (dword j of row q at j ^ (swz(q) << 2)).  No VGPR holds the
// window on the way.  Chunks wholly past the frame are not loaded (the
// source masks the bytes past caplen instead).  The loads are nontemporal
// (aux 2): a window's lines are read once, and as L2-allocating loads
// they pushed out the packets' first lines that the late chunk loads had
// just brought in for the walkers (C4: 308.6 -> 259.4 B/packet read, 40.5M
// -> 34.0M 128-byte requests per launch against a line floor of 262.9;
// kernel time unchanged).  abase: this lane's aligned
// window start in HBM; rem: bytes from there to the frame's aligned end (0:
// the lane takes no window).
__device__ __forceinline__ uint32_t swz_of(uint32_t q, int cpp) { return (q >> 1) & (uint32_t)(cpp - 1); }

template <int WIN>
__device__ __forceinline__ void stage_glds(uint32_t *wwin, uint64_t abase, uint32_t rem, int lane)
{
	constexpr int CPP = WIN / 16, PER = 64 / CPP;
	static_assert(CPP * PER == 64, "a window size whose slots tile a wave");
	const uint32_t lo = (uint32_t)abase;
	// the high address dword (a 48-bit VA) shares its word with min(rem, 0xFFFF)
	const uint32_t hr = (uint32_t)(abase >> 32) | (rem < 0xFFFFu ? rem : 0xFFFFu) << 16;
#pragma unroll 2
	for (int r = 0; r < CPP; r++) {
		const int q = r * PER + lane / CPP;
		const uint32_t alo = __shfl(lo, q, 64), ahr = __shfl(hr, q, 64);
		const uint32_t c = ((uint32_t)lane % CPP) ^ swz_of((uint32_t)q, CPP);
		if (16 * c < (ahr >> 16)) {
			const uint64_t a = ((uint64_t)(ahr & 0xFFFFu) << 32 | alo) + 16 * c;
			__builtin_amdgcn_global_load_lds((const void *)a,
							 (__attribute__((address_space(3))) void *)(wwin + r * 256), 16, 0,
							 2);
		}
	}
	// the DMA's LDS writes are ordered for this wave's reads by its vmcnt only
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void wave_sync_lds()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ICMPv4 checksum helpers (calc_csum over the whole message, csum.h:12-27).
// Only whether the checksum is zero is kept (NSD_F_ICMP_BAD).  Sums run over
// the 16-bit halves of 16-byte aligned loads with the bytes outside the
// message masked off.  For a message at an odd address that weights every
// byte by 256 relative to the reference's LE words, i.e. multiplies the sum
// by 256 mod 0xFFFF (65536 = 1), so the folded sum is 0xFFFF exactly when the
// reference's is (RFC 1071 byte-order independence) and the checksum is zero
// exactly when the reference's is.  Partial sums may be folded early: folding
// keeps the value mod 0xFFFF and keeps it non-zero.

// byte mask of the dword at aligned position p for message bytes [s0, endb)
__device__ __forceinline__ uint32_t msg_mask(uint32_t p, uint32_t s0, uint32_t endb)
{
	uint32_t m = 0xFFFFFFFFu;
	if (s0 > p)
		m = s0 >= p + 4 ? 0u : m << (8 * (s0 - p));
	if (endb < p + 4)
		m = endb <= p ? 0u : m & (0xFFFFFFFFu >> (8 * (p + 4 - endb)));
	return m;
}

// acc + low half + high half (v_sad_u16 against zero)
__device__ __forceinline__ uint32_t sum_halves(uint32_t x, uint32_t acc)
{
	return __builtin_amdgcn_sad_u16(x, 0u, acc);
}

// chunk at aligned position lo, bytes outside [s0, endb) masked per lane
__device__ __forceinline__ uint32_t csum_chunk(const uint4 &v, uint32_t lo, uint32_t s0, uint32_t endb)
{
	uint32_t acc = sum_halves(v.x & msg_mask(lo, s0, endb), 0u);
	acc = sum_halves(v.y & msg_mask(lo + 4, s0, endb), acc);
	acc = sum_halves(v.z & msg_mask(lo + 8, s0, endb), acc);
	return sum_halves(v.w & msg_mask(lo + 12, s0, endb), acc);
}

__device__ __forceinline__ uint16_t csum_final(uint32_t sum)
{
	sum = (sum >> 16) + (sum & 0xffff);
	sum += (sum >> 16);
	return (uint16_t)~sum;
}

// Streaming record store: nontemporal (written once, read by the host or a
// later kernel), measured 6 % faster than a plain store in the pass-1 access
// shape (tools/bw: 72 B read + 16 B written per packet).
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_rec(uint4 *rec, uint32_t i, uint4 r)
{
	const v4u v = { r.x, r.y, r.z, r.w };
	__builtin_nontemporal_store(v, (v4u *)(rec + i));
}

// The record of packet i in the launch's record form: the 16-byte nsd_rec,
// or (CR) the 8-byte nsd_crec - the same results without the cursors a
// renderer re-derives from the bytes: the first 6 ids, the layer count in
// nlayers for 7..12 layers (ids 6..11 in the packet's side word), or the ext
// slot of a longer chain
__device__ __forceinline__ uint2 crec_of(const WalkOut &w)
{
	const bool more = w.n > NSD_REC_MAX_LAYERS;
	const uint32_t nf = (more ? NSD_N_EXT : w.n) | w.flags;
	const uint32_t rs = more && !w.ext_on ? w.n : 0u;
	return make_uint2(w.ext_on ? w.slot : w.chain, w.ip_csum | nf << 16 | rs << 24);
}

template <bool CR>
__device__ __forceinline__ void put_rec(void *rec, uint32_t i, const WalkOut &w)
{
	if constexpr (CR) {
		const uint2 r = crec_of(w);
		__builtin_nontemporal_store(v2u{ r.x, r.y }, (v2u *)rec + i);
	} else {
		store_rec((uint4 *)rec, i, pack_record(w));
	}
}

// The fused tile loop's pending-list entries and, without the record ring
// (the plain build, RING false), its compact records, held one tile: a
// tile's stores are issued after the next tile's
// chunk wait and before its prefetch loads, so the wait that precedes each
// tile (vmcnt(0): its chunks are the youngest loads) finds them issued a
// whole tile earlier (C3 -1 %).  (Nontemporal stores: as sc1 stores, the
// split kernel's choice below, C3 ran 1.5 % slower.)  Measured on the C3
// tile phase without its walk: the record stores cost 0.07
// of its 0.35 ms however they are issued - every tile or every fourth in 4x
// larger pieces, 8 or 16 bytes per lane, held or not - i.e. the writes'
// interleaving with the scattered window reads in HBM, not a wait in this
// loop.  The 16-byte form stores at once (held, its four words spill the
// fused kernel's registers).
template <bool CR>
struct HeldSt {
	uint2 r;          // the compact record (nsd_crec)
	uint32_t ri;      // packet index of the record; ~0: none
	uint64_t pe;      // pending-list entry
	uint32_t pp;      // its slot; ~0: none
	__device__ __forceinline__ void hold_rec(uint32_t i, uint2 rv, bool on)
	{
		ri = on ? i : 0xFFFFFFFFu;
		r = rv;
	}
	__device__ __forceinline__ void hold_pend(uint64_t *wq, uint64_t e, uint32_t slot)
	{
		if constexpr (!CR) {
			if (slot != 0xFFFFFFFFu)
				wq[slot] = e;   // (not held either, as the 16-byte record)
			return;
		}
		pe = e;
		pp = slot;
	}
	__device__ __forceinline__ void flush(void *rec, uint64_t *wq)
	{
		if constexpr (!CR)
			return;
		if (ri != 0xFFFFFFFFu)
			__builtin_nontemporal_store(v2u{ r.x, r.y }, (v2u *)rec + ri);
		if (pp != 0xFFFFFFFFu)
			wq[pp] = pe;
		ri = pp = 0xFFFFFFFFu;
	}
};

// The split fast loop's stores are inline-asm vector stores: hipcc's
// waitcnt pass treats the vector-memory counter as
// out of order while loads and stores are both pending and then waits
// vmcnt(0) for a tile's chunks - for every later chunk load and every store
// too, which defeats a deeper prefetch.  It does not see these stores, so its
// waits count the loop's loads alone; loads complete in order among
// themselves, so a wait that leaves N later loads outstanding still covers
// the load it waits for, whatever the stores do.  Their completion is ours:
// drain_stores() before anything reads what they wrote.  The compact record
// stores use the sc1 policy (written through, the line dropped from the
// XCD's L2; MI355X_MICROARCH.md "stores of each flavour"): C2 0.2069 - 0.2092
// -> 0.2036 - 0.2049 ms against nontemporal stores on one box (records are
// read by the host or another kernel, never by this wave again); the 16-byte
// records stay nontemporal (sc1 there: +12 %).  A store of more
// than 8 bytes reads its data registers over two cycles, and hipcc's hazard
// recognizer does not know an asm statement is such a store: the next VALU
// could overwrite the data before it is read (gfx9's 12-dword store hazard;
// without the wait state a build with three tiles in flight wrote corrupt
// list entries and faulted the GPU).  The 16-byte forms end in s_nop 1.
__device__ __forceinline__ void st_b32(uint32_t *p, uint32_t v)
{
	asm volatile("global_store_dword %0, %1, off" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_b128(uint4 *p, uint4 x)
{
	const v4u v = { x.x, x.y, x.z, x.w };
	asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void drain_stores()
{
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <bool CR>
__device__ __forceinline__ void put_rec_st(void *rec, uint32_t i, const WalkOut &w)
{
	if constexpr (CR) {
		const uint2 r = crec_of(w);
		const v2u v = { r.x, r.y };
		asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"((v2u *)rec + i), "v"(v) : "memory");
	} else {
		const uint4 r = pack_record(w);
		const v4u v = { r.x, r.y, r.z, r.w };
		// (16-byte records stay nontemporal: with sc1 0.2667 - 0.2677 ms
		// against 0.2370 - 0.2378)
		asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" ::"v"((uint4 *)rec + i), "v"(v) : "memory");
	}
}

// byte offset of packet i's nflags in the record array
template <bool CR>
__device__ __forceinline__ size_t nflags_at(uint32_t i)
{
	return CR ? (size_t)i * 8 + 6 : (size_t)i * 16 + 10;
}

// Per-wave flag counters: wave-uniform (ballot + popcount, scalar registers);
// only the byte count is per lane.
struct FlagCnt {
	uint32_t pkts = 0, ipbad = 0, icmpbad = 0, host = 0, ext = 0, ovf = 0, trim = 0;
	uint64_t bytes = 0;
	__device__ __forceinline__ static uint32_t pc(bool c) { return (uint32_t)__popcll(__ballot(c)); }
	__device__ __forceinline__ void add(const WalkOut &w, uint32_t caplen, bool on)
	{
		pkts += pc(on);
		ipbad += pc(on && w.ip_csum != 0);
		icmpbad += pc(on && (w.flags & NSD_F_ICMP_BAD));
		host += pc(on && (w.flags & NSD_F_HOST));
		ext += pc(on && w.need_ext);
		ovf += pc(on && (w.flags & NSD_F_OVERFLOW));
		trim += pc(on && w.tail < caplen);
		if (on)
			bytes += caplen;
	}
	// -> block LDS counters
	__device__ __forceinline__ void flush(unsigned long long *s_cnt, int lane) const
	{
		const uint32_t vals[7] = { pkts, ipbad, icmpbad, host, ext, ovf, trim };
		const int idx[7] = { NSD_CNT_PKTS, NSD_CNT_IP_BAD, NSD_CNT_ICMP_BAD, NSD_CNT_HOST,
				     NSD_CNT_EXT, NSD_CNT_OVERFLOW, NSD_CNT_TRIM };
		if (lane == 0) {
#pragma unroll
			for (int k = 0; k < 7; k++)
				if (vals[k])
					atomicAdd(&s_cnt[idx[k]], (unsigned long long)vals[k]);
		}
		const uint64_t b = wave_sum64(bytes);
		if (lane == 0 && b)
			atomicAdd(&s_cnt[NSD_CNT_BYTES], (unsigned long long)b);
	}
};

__device__ __forceinline__ void block_init(unsigned long long *s_cnt, uint8_t *s_lay3)
{
	for (int k = threadIdx.x; k < NSD_NCOUNTERS; k += BLOCK)
		s_cnt[k] = 0;
	for (int k = threadIdx.x; k < 256; k += BLOCK)
		s_lay3[k] = c_lay3[k];
	__syncthreads();
}

__device__ __forceinline__ void block_flush(unsigned long long *s_cnt, unsigned long long *counters)
{
	__syncthreads();
	for (int k = threadIdx.x; k < NSD_NCOUNTERS; k += BLOCK)
		if (s_cnt[k])
			atomicAdd(&counters[k], s_cnt[k]);
}

// Pending ICMPv4 checksums: entry = packet index | message offset << 32 |
// message length << 48 (offsets and lengths are < 65536).  Each wave of a
// block keeps one list (room for every packet it visits).
__device__ __forceinline__ uint64_t pend_entry(uint32_t i, uint32_t off, uint32_t len)
{
	return (uint64_t)i | (uint64_t)(off & 0xFFFF) << 32 | (uint64_t)(len & 0xFFFF) << 48;
}

} // namespace nsd

#endif
