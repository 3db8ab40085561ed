// nsd_flow_table.h - the flow table's own kernels (reset, update, commit,
// export) and what every later section of nsd_flow.hip uses of a table: its
// rows, the key helpers, the read-only probe and the wave-aggregated cursor.
// Device code of one translation unit: nsd_flow.hip includes it, then
// nsd_flow_conv.h and nsd_flow_expire.h.  The table's layout and the rules of
// its slots are in nsd_flow.hip's head comment.
#ifndef NSD_FLOW_TABLE_H
#define NSD_FLOW_TABLE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nsd_flow.h"
#include "nsd_internal.h"

namespace nsdflow {

// (MAX_N, the most packets of one update, is nsd_internal.h's: nsd_flow_cpu.cpp checks it too)
constexpr uint32_t EMPTY = 0xFFFFFFFFu, OCCUPIED = 0xFFFFFFFEu, NOSLOT = 0xFFFFFFFFu;
constexpr int BLOCK = 256;

struct Cnt {
	uint64_t pkts, bytes, first, last;
	uint32_t flags, pad;
};
static_assert(sizeof(Cnt) == 40, "cnt row");
static_assert(sizeof(nsd_flow) == 72, "nsd_flow");
static_assert(sizeof(nsd_flowt) == 88 && offsetof(nsd_flowt, t_first) == 72, "nsd_flowt");
static_assert(offsetof(nsd_flowt, pkts) == offsetof(nsd_flow, pkts) && offsetof(nsd_flowt, last) == offsetof(nsd_flow, last),
	      "nsd_flowt begins as nsd_flow");

// what the kernels need of a table
struct Tab {
	uint32_t *state;
	uint64_t *key;
	Cnt *cnt;
	uint64_t *stats;
	uint32_t slots;
	uint64_t *tm;   // two words per slot, or nullptr: a plain table
};

// one update's inputs
struct In {
	const uint8_t *frames;
	const uint64_t *desc;
	const nsd_rec *rec;
	const uint32_t *ext;
	uint32_t ext_words;
	uint32_t n;
	uint64_t base;
	const uint64_t *ts;   // packet i's timestamp (the timed update), else nullptr
};

__device__ __forceinline__ int packet_key(const In &in, uint32_t i, Key &k, uint32_t &tflags, uint32_t &caplen)
{
	const uint4 q = ((const uint4 *)in.rec)[i];
	nsd_rec r;
	memcpy(&r, &q, sizeof(r));
	const uint64_t d = in.desc[i];
	caplen = NSD_DESC_CAPLEN(d);
	return flow_key(r, in.ext, in.ext_words, in.frames + NSD_DESC_OFF(d), caplen, k, tflags);
}

template <class T>
__device__ __forceinline__ void add_rlx(T *p, T v)
{
	(void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void accumulate(Cnt *c, uint64_t pkts, uint64_t bytes, uint64_t first, uint64_t last,
					   uint32_t flags)
{
	add_rlx(&c->pkts, pkts);
	add_rlx(&c->bytes, bytes);
	(void)__hip_atomic_fetch_min(&c->first, first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_max(&c->last, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (flags)
		(void)__hip_atomic_fetch_or(&c->flags, flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the times of a slot of a timed table: min / max, whatever the order of the packets
__device__ __forceinline__ void accumulate_times(uint64_t *tm, uint64_t t_first, uint64_t t_last)
{
	(void)__hip_atomic_fetch_min(&tm[0], t_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_max(&tm[1], t_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the counters of no packets: what the sums, minima and maxima start from
__device__ __forceinline__ Cnt empty_cnt()
{
	Cnt c;
	c.pkts = c.bytes = c.last = 0;
	c.first = UINT64_MAX;
	c.flags = c.pad = 0;
	return c;
}

// a slot without a flow
__device__ __forceinline__ void clear_slot(const Tab &t, uint64_t s)
{
	t.state[s] = EMPTY;
	t.cnt[s] = empty_cnt();
	if (t.tm) {
		t.tm[2 * s] = UINT64_MAX;
		t.tm[2 * s + 1] = 0;
	}
}

// the five key words of a slot
__device__ __forceinline__ void load_key(const Tab &t, uint32_t s, Key &k)
{
	const uint64_t *kp = t.key + 5ull * s;
	for (int j = 0; j < 5; j++)
		k.w[j] = kp[j];
}
__device__ __forceinline__ void store_key(const Tab &t, uint32_t s, const Key &k)
{
	uint64_t *kp = t.key + 5ull * s;
	for (int j = 0; j < 5; j++)
		kp[j] = k.w[j];
}

// The nine words of an nsd_flow row (an nsd_flowt row begins with them) from a
// flow's key and counters: the flags go into word 4, which the key leaves zero
// from bit 48.
__device__ __forceinline__ void store_flow_row(uint64_t *o, const Key &k, const Cnt &c)
{
	o[0] = k.w[0];
	o[1] = k.w[1];
	o[2] = k.w[2];
	o[3] = k.w[3];
	o[4] = k.w[4] | (uint64_t)(c.flags & 0xFFu) << 48;
	o[5] = c.pkts;
	o[6] = c.bytes;
	o[7] = c.first;
	o[8] = c.last;
}

// memcmp of the 40 key bytes: the words are little-endian images of them
__device__ __forceinline__ bool key_bytes_less(const Key &a, const Key &b)
{
	for (int j = 0; j < 5; j++)
		if (a.w[j] != b.w[j])
			return __builtin_bswap64(a.w[j]) < __builtin_bswap64(b.w[j]);
	return false;
}

// the reverse of a key: src / dst and sport / dport swapped, l3 / l4 kept
__device__ __forceinline__ void reverse_key(const Key &k, Key &r)
{
	r.w[0] = k.w[2];
	r.w[1] = k.w[3];
	r.w[2] = k.w[0];
	r.w[3] = k.w[1];
	r.w[4] = (k.w[4] & ~0xFFFFFFFFull) | (k.w[4] & 0xFFFFu) << 16 | (k.w[4] >> 16 & 0xFFFFu);
}

// The slot that holds key r in a table whose slots are EMPTY or OCCUPIED
// (after the commit), or NOSLOT: the update's probe, read-only.  EMPTY ends
// it, and the slot count bounds it (a table without an empty slot).
__device__ __forceinline__ uint32_t find_key(const Tab &t, const Key &r)
{
	const uint32_t mask = t.slots - 1;
	uint32_t p = (uint32_t)key_hash(r) & mask;
#pragma unroll 1
	for (uint32_t probes = 0; probes < t.slots; probes++, p = (p + 1) & mask) {
		const uint32_t v = t.state[p];
		if (v == EMPTY)
			break;
		if (v != OCCUPIED)
			continue;
		Key o;
		load_key(t, p, o);
		if (key_eq(o, r))
			return p;
	}
	return NOSLOT;
}

// The wave-aggregated cursor: a position for every lane of `m` (a ballot, not
// zero) from one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ uint64_t wave_cursor(uint32_t *cursor, uint64_t m, uint32_t lane)
{
	uint32_t at = 0;
	if (lane == 0)
		at = __hip_atomic_fetch_add(cursor, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	at = __shfl(at, 0, 64);
	return (uint64_t)at + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(BLOCK) void flow_reset(Tab t)
{
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.slots; s += stride)
		clear_slot(t, s);
	if (blockIdx.x == 0 && threadIdx.x < NSD_FLOW_NSTATS)
		t.stats[threadIdx.x] = 0;
}

// A block's own sums in LDS: AGG_N entries, direct-mapped by the table
// slot.  An entry belongs to the first slot that takes it (one LDS CAS on its
// tag) until the block ends, when its sums go to the table with one set of
// atomics; a slot that finds its entry taken by another adds to the table
// itself.  Heavy hitters meet the table once per block instead of once per
// packet; first / last are kept as packet indices of the launch.
constexpr uint32_t AGG_N = 512;
struct Agg {
	uint32_t tag[AGG_N], pkts[AGG_N], first[AGG_N], last[AGG_N], flags[AGG_N];
	unsigned long long bytes[AGG_N];
};
// The timed update's entries carry the flow's two times as well.  They are
// whole 64-bit values of any epoch (0 and UINT64_MAX included, and a file's
// need not ascend), so there is no 32-bit form of them as there is of first /
// last: 64-bit LDS min / max, 8 KB more per block.
struct AggTimes {
	unsigned long long tmin[AGG_N], tmax[AGG_N];
};
template <bool TIMED>
struct AggMem {
	Agg a;
};
template <>
struct AggMem<true> {
	Agg a;
	AggTimes tt;
};

template <bool TIMED>
__device__ __forceinline__ void add_flow(const Tab &t, const In &in, AggMem<TIMED> *mem, uint32_t slot, uint32_t pkts,
					 uint32_t bytes, uint32_t first, uint32_t last, uint32_t flags, uint64_t ts)
{
	Agg *agg = &mem->a;
	const uint32_t e = slot & (AGG_N - 1);
	const uint32_t old = atomicCAS(&agg->tag[e], NOSLOT, slot);
	if (old == NOSLOT || old == slot) {
		atomicAdd(&agg->pkts[e], pkts);
		atomicAdd(&agg->bytes[e], (unsigned long long)bytes);
		atomicMin(&agg->first[e], first);
		atomicMax(&agg->last[e], last);
		if (flags)
			atomicOr(&agg->flags[e], flags);
		if constexpr (TIMED) {
			atomicMin(&mem->tt.tmin[e], (unsigned long long)ts);
			atomicMax(&mem->tt.tmax[e], (unsigned long long)ts);
		}
		return;
	}
	accumulate(&t.cnt[slot], pkts, bytes, in.base + first, in.base + last, flags);
	if constexpr (TIMED)
		accumulate_times(t.tm + 2ull * slot, ts, ts);
}

// One packet per lane, grid-stride; the rounds are wave-uniform, so the
// stats are ballots over whole waves.  The block sums in LDS (above) and
// adds its entries to the table after its last packet.  TIMED: a timed table
// and in.ts; a packet that is counted (it found its flow's slot) gives its
// timestamp to the flow's minimum and maximum, the others' are not read.
template <bool TIMED>
__global__ __launch_bounds__(BLOCK) void flow_update(Tab t, In in)
{
	__shared__ AggMem<TIMED> agg_mem;
	Agg *agg = &agg_mem.a;
	for (uint32_t e = threadIdx.x; e < AGG_N; e += BLOCK) {
		agg->tag[e] = NOSLOT;
		agg->pkts[e] = agg->last[e] = agg->flags[e] = 0;
		agg->first[e] = 0xFFFFFFFFu;
		agg->bytes[e] = 0;
		if constexpr (TIMED) {
			agg_mem.tt.tmin[e] = ~0ull;
			agg_mem.tt.tmax[e] = 0;
		}
	}
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t mask = t.slots - 1;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	uint32_t w_keyed = 0, w_noip = 0, w_skip = 0, w_full = 0, w_new = 0, w_pkts = 0;
#pragma unroll 1
	for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); i0 < in.n; i0 += stride) {
		const uint64_t i = i0 + lane;
		const bool live = i < in.n;
		Key k;
		uint32_t tflags = 0, caplen = 0;
		int st = -1;
		if (live)
			st = packet_key(in, (uint32_t)i, k, tflags, caplen);
		const bool keyed = st == K_KEYED;
		uint32_t slot = NOSLOT;
		bool fresh = false;
		if (keyed) {
			uint32_t s = (uint32_t)key_hash(k) & mask;
#pragma unroll 1
			for (uint32_t probes = 0; probes < t.slots; probes++, s = (s + 1) & mask) {
				uint32_t v = __hip_atomic_load(&t.state[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (v == EMPTY) {
					uint32_t expect = EMPTY;
					if (__hip_atomic_compare_exchange_strong(&t.state[s], &expect, (uint32_t)i,
										 __ATOMIC_RELAXED, __ATOMIC_RELAXED,
										 __HIP_MEMORY_SCOPE_AGENT)) {
						slot = s;
						fresh = true;
						break;
					}
					v = expect;   // somebody else's claim: compare with it
				}
				bool same = false;
				if (v == OCCUPIED) {
					// (load_key written out: through the call the compiler orders
					// two moves of this kernel differently, and its code is pinned)
					Key o;
					const uint64_t *kp = t.key + 5ull * s;
					for (int j = 0; j < 5; j++)
						o.w[j] = kp[j];
					same = key_eq(o, k);
				} else if (v < in.n) {
					// claimed in this launch by packet v: its key, from the inputs
					Key o;
					uint32_t of, oc;
					same = packet_key(in, v, o, of, oc) == K_KEYED && key_eq(o, k);
				}
				if (same) {
					slot = s;
					break;
				}
			}
		}
		const bool found = slot != NOSLOT;
		w_pkts += (uint32_t)__popcll(__ballot(live));
		w_keyed += (uint32_t)__popcll(__ballot(keyed));
		w_noip += (uint32_t)__popcll(__ballot(st == K_NOIP));
		w_skip += (uint32_t)__popcll(__ballot(st == K_SKIPPED));
		w_full += (uint32_t)__popcll(__ballot(keyed && !found));
		w_new += (uint32_t)__popcll(__ballot(fresh));
		if (found) {
			uint64_t ts = 0;
			if constexpr (TIMED)
				ts = in.ts[i];
			add_flow<TIMED>(t, in, &agg_mem, slot, 1, caplen, (uint32_t)i, (uint32_t)i, tflags, ts);
		}
	}
	if (lane == 0) {
		if (w_pkts)
			add_rlx(&t.stats[NSD_FLOW_ST_PKTS], (uint64_t)w_pkts);
		if (w_keyed)
			add_rlx(&t.stats[NSD_FLOW_ST_KEYED], (uint64_t)w_keyed);
		if (w_noip)
			add_rlx(&t.stats[NSD_FLOW_ST_NOIP], (uint64_t)w_noip);
		if (w_skip)
			add_rlx(&t.stats[NSD_FLOW_ST_SKIPPED], (uint64_t)w_skip);
		if (w_full)
			add_rlx(&t.stats[NSD_FLOW_ST_FULL], (uint64_t)w_full);
		if (w_new)
			add_rlx(&t.stats[NSD_FLOW_ST_FLOWS], (uint64_t)w_new);
	}
	__syncthreads();
	for (uint32_t e = threadIdx.x; e < AGG_N; e += BLOCK) {
		const uint32_t slot = agg->tag[e];
		if (slot < t.slots) {
			accumulate(&t.cnt[slot], agg->pkts[e], agg->bytes[e], in.base + agg->first[e], in.base + agg->last[e],
				   agg->flags[e]);
			if constexpr (TIMED)
				accumulate_times(t.tm + 2ull * slot, agg_mem.tt.tmin[e], agg_mem.tt.tmax[e]);
		}
	}
}

// the key of the claiming packet into key[slot]; the slot is OCCUPIED from now on
__device__ __forceinline__ void commit_slot(const Tab &t, const In &in, uint32_t s)
{
	const uint32_t v = t.state[s];
	if (v >= in.n)   // EMPTY, OCCUPIED (or nothing of this launch)
		return;
	Key k;
	uint32_t tf, cl;
	(void)packet_key(in, v, k, tf, cl);
	// (store_key written out, as load_key in the update: this kernel's listing is pinned too)
	uint64_t *kp = t.key + 5ull * s;
	for (int j = 0; j < 5; j++)
		kp[j] = k.w[j];
	t.state[s] = OCCUPIED;
}

// (a scan of `state`: a list of the claimed slots, appended to by the update,
// made an all-insert update 15-20 % slower and a warm one no faster -
// DESIGN.md "Flow table")
__global__ __launch_bounds__(BLOCK) void flow_commit(Tab t, In in)
{
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.slots; s += stride)
		commit_slot(t, in, (uint32_t)s);
}

// Occupied slots packed into `out` through a wave-aggregated cursor (*count,
// zeroed before the launch); rows past `max` are counted, not written.  TS:
// nsd_flowt rows, the slot's two times after the nine words of nsd_flow.
template <bool TS>
__global__ __launch_bounds__(BLOCK) void flow_export(Tab t, uint64_t *out, uint32_t max, uint32_t *count,
						     uint64_t *stats_out)
{
	constexpr uint64_t ROW = TS ? 11 : 9;
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
#pragma unroll 1
	for (uint64_t s0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); s0 < t.slots; s0 += stride) {
		const uint64_t s = s0 + lane;
		const bool occ = s < t.slots && t.state[s] == OCCUPIED;
		const uint64_t m = __ballot(occ);
		if (!m)
			continue;
		const uint64_t pos = wave_cursor(count, m, lane);
		if (occ && pos < max) {
			// (store_flow_row's words written out, the key straight from the table:
			// with the whole key loaded first the export of a nearly empty table
			// measured 2 - 4 us slower, profiles/flow_split)
			const uint64_t *kp = t.key + 5ull * s;
			const Cnt c = t.cnt[s];
			uint64_t *o = out + ROW * pos;
			o[0] = kp[0];
			o[1] = kp[1];
			o[2] = kp[2];
			o[3] = kp[3];
			o[4] = kp[4] | (uint64_t)(c.flags & 0xFFu) << 48;
			o[5] = c.pkts;
			o[6] = c.bytes;
			o[7] = c.first;
			o[8] = c.last;
			if constexpr (TS) {
				o[9] = t.tm[2 * s];
				o[10] = t.tm[2 * s + 1];
			}
		}
	}
	if (blockIdx.x == 0 && threadIdx.x < NSD_FLOW_NSTATS)
		stats_out[threadIdx.x] = t.stats[threadIdx.x];
}

} // namespace nsdflow

#endif /* NSD_FLOW_TABLE_H */
