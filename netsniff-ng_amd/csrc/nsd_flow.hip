// nsd_flow.hip - per-flow statistics on the device: a flow table in HBM over
// dissected batches (include/netsniff_dissect.h "flow table").  What flowtop
// shows per conversation (flowtop.c: the per-flow packet and byte counters it
// reads from conntrack) is here aggregated from the records of a batch walk,
// so a 16 M-packet batch leaves the device as a few thousand rows.
//
// Table: open addressing, linear probing, three arrays indexed by slot:
//   state[slots] u32 : EMPTY, OCCUPIED (key[slot] was stored by an earlier
//                      launch), or the index p of a packet of the *current*
//                      update: the flow is new in this launch and its key is
//                      packet p's, which any lane re-derives from the launch's
//                      own inputs (nobody writes those);
//   key[slots]  40 B : five u64 words (nsd_flow.h Key);
//   cnt[slots]  40 B : pkts, bytes, first, last (u64), flags (u32);
//   tm[slots]   16 B : t_first, t_last (u64), the smallest / largest capture
//                      timestamp of the flow's packets: a timed table only
//                      (nsd_flow_create_timed, the header's "flow times"); a
//                      plain table has no such array and its kernels are the
//                      instantiations that never look for one.
//
// No lane ever waits on another lane's store: a slot is claimed with one
// 32-bit CAS EMPTY -> packet index, and what a lane needs to compare against
// a claimed slot is already in memory before the launch (the claimer's
// packet).  The commit kernel, after the update kernel on the same stream,
// stores the keys of the slots claimed in that launch and marks them
// OCCUPIED.  No spin loops, no published flags, no fences; every probe loop
// is bounded by the slot count.  (The update's blocks sum in LDS first and
// meet at two block barriers, which every thread reaches.)
//
// A flow is in the table wholly or not at all: slots never change owner, so
// the slots a flow's packet found taken by other flows stay so for every
// later packet of that flow, and a packet that meets its flow's slot matches.
// (Expiry, below, keeps this true for the update: it never empties a slot in
// place but rebuilds the table from its survivors between two updates.)
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "nsd_flow.h"
#include "nsd_internal.h"

namespace nsdflow {

constexpr uint32_t EMPTY = 0xFFFFFFFFu, OCCUPIED = 0xFFFFFFFEu, NOSLOT = 0xFFFFFFFFu;
constexpr uint32_t MAX_N = 0xFFFFFFF0u;
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

// a slot without a flow: what the sums, minima and maxima start from
__device__ __forceinline__ void clear_slot(const Tab &t, uint64_t s)
{
	t.state[s] = EMPTY;
	Cnt c;
	c.pkts = c.bytes = c.last = 0;
	c.first = UINT64_MAX;
	c.flags = c.pad = 0;
	t.cnt[s] = c;
	if (t.tm) {
		t.tm[2 * s] = UINT64_MAX;
		t.tm[2 * s + 1] = 0;
	}
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
		uint32_t at = 0;
		if (lane == 0)
			at = __hip_atomic_fetch_add(count, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		at = __shfl(at, 0, 64);
		const uint64_t pos = (uint64_t)at + (uint32_t)__popcll(m & ((1ull << lane) - 1));
		if (occ && pos < max) {
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

// ---- conversations and top-k ------------------------------------------------
// A flow and its reverse (src / dst and sport / dport swapped) are one
// conversation, owned by the direction seen first (the header's "pairing").
// These kernels run after the commit on the table's stream and only read the
// table: state is EMPTY or OCCUPIED, no atomics on it, no fences.
//
// Workspace: a CONV_HDR-byte header, then by candidate index four arrays of `slots` entries: hi u64 | lo u64 (the sort
// key, larger is better) | slot u32 | rev u32 (the reverse's slot or NOSLOT).
// conv_init zeroes the header: a kernel, not hipMemsetAsync - a memset
// captured into a HIP graph does not reliably run on replay (DESIGN.md 4.1,
// 4.8), and a header left as it was sends the later kernels past the
// candidate arrays.  They bound what they read from the workspace by `slots`
// all the same.
constexpr size_t CONV_HDR = 2048;
constexpr int CONV_DIGITS = 16;   // 8-bit digits of the 128-bit key, most significant first

struct ConvHdr {
	uint32_t ncand;      // candidates = conversations (conv_pair's cursor)
	uint32_t rem;        // rows still wanted among the candidates that match `pre`
	uint32_t n_above;    // conv_gather's cursor of rows above the threshold
	uint32_t n_tied;     // ... and of rows equal to it
	uint64_t pre[2];     // hi, lo: the digits decided so far; in the end the k-th key
	uint64_t any1[2];    // OR of the keys
	uint64_t any0[2];    // OR of the keys' complements
	uint32_t bins[256];
};
static_assert(sizeof(ConvHdr) <= CONV_HDR && offsetof(ConvHdr, bins) % 16 == 0, "conv header");

struct ConvWs {
	ConvHdr *h;
	uint64_t *hi, *lo;
	uint32_t *slot, *rev;
	uint32_t slots;
};

__global__ __launch_bounds__(BLOCK) void conv_init(ConvWs w)
{
	for (uint32_t i = threadIdx.x; i < sizeof(ConvHdr) / 4; i += BLOCK)
		((uint32_t *)w.h)[i] = 0;
}

// the candidates: conv_pair's cursor, never more than the slots
__device__ __forceinline__ uint32_t conv_ncand(const ConvWs &w)
{
	const uint32_t n = w.h->ncand;
	return n < w.slots ? n : w.slots;
}

__device__ __forceinline__ void load_key(const Tab &t, uint32_t s, Key &k)
{
	const uint64_t *kp = t.key + 5ull * s;
	for (int j = 0; j < 5; j++)
		k.w[j] = kp[j];
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

// One slot per lane, grid-stride.  The slot that owns its conversation emits
// a candidate through a wave-aggregated cursor; the OR of the keys and of
// their complements (which digits differ at all) is combined per thread, then
// per block in LDS, and reaches the header once per block.
__global__ __launch_bounds__(BLOCK) void conv_pair(Tab t, ConvWs w, int by)
{
	__shared__ unsigned long long red[4];
	if (threadIdx.x < 4)
		red[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	uint64_t o1h = 0, o1l = 0, o0h = 0, o0l = 0;
#pragma unroll 1
	for (uint64_t s0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); s0 < t.slots; s0 += stride) {
		const uint64_t s = s0 + lane;
		const bool occ = s < t.slots && t.state[s] == OCCUPIED;
		bool own = false;
		uint32_t rev = NOSLOT;
		uint64_t hi = 0, lo = 0;
		if (occ) {
			Key k, r;
			load_key(t, (uint32_t)s, k);
			reverse_key(k, r);
			const Cnt c = t.cnt[s];
			uint64_t metric = by == NSD_CONV_BY_PKTS ? c.pkts : c.bytes;
			own = true;
			if (!key_eq(k, r)) {
				rev = find_key(t, r);
				if (rev != NOSLOT) {
					const Cnt d = t.cnt[rev];
					own = c.first < d.first || (c.first == d.first && key_bytes_less(k, r));
					metric += by == NSD_CONV_BY_PKTS ? d.pkts : d.bytes;
				}
			}
			// (the owner's `first` is the conversation's: the smaller of the two)
			if (by == NSD_CONV_BY_FIRST)
				hi = ~c.first;
			else
				hi = metric, lo = ~c.first;
		}
		const uint64_t m = __ballot(own);
		if (!m)
			continue;
		uint32_t at = 0;
		if (lane == 0)
			at = __hip_atomic_fetch_add(&w.h->ncand, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		at = __shfl(at, 0, 64);
		if (own) {
			const uint64_t pos = (uint64_t)at + (uint32_t)__popcll(m & ((1ull << lane) - 1));
			if (pos < t.slots) {
				w.hi[pos] = hi;
				w.lo[pos] = lo;
				w.slot[pos] = (uint32_t)s;
				w.rev[pos] = rev;
			}
			o1h |= hi;
			o1l |= lo;
			o0h |= ~hi;
			o0l |= ~lo;
		}
	}
	if (o1h | o0h) {   // (a thread that emitted has a bit in one of the two)
		atomicOr(&red[0], (unsigned long long)o1h);
		atomicOr(&red[1], (unsigned long long)o1l);
		atomicOr(&red[2], (unsigned long long)o0h);
		atomicOr(&red[3], (unsigned long long)o0l);
	}
	__syncthreads();
	if (threadIdx.x < 4 && red[threadIdx.x]) {
		uint64_t *dst = threadIdx.x < 2 ? &w.h->any1[threadIdx.x] : &w.h->any0[threadIdx.x - 2];
		(void)__hip_atomic_fetch_or(dst, (uint64_t)red[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// digit d (0 = most significant) of a key, and the key's digits above it
__device__ __forceinline__ uint32_t conv_digit(uint64_t hi, uint64_t lo, int d)
{
	return (uint32_t)((d < 8 ? hi : lo) >> (8 * (7 - (d & 7)))) & 255u;
}
__device__ __forceinline__ bool conv_above_match(uint64_t hi, uint64_t lo, const uint64_t pre[2], int d)
{
	// mask of the digits 0 .. d-1
	const uint64_t mh = d >= 8 ? ~0ull : d == 0 ? 0ull : ~0ull << (8 * (8 - d));
	const uint64_t ml = d <= 8 ? 0ull : ~0ull << (8 * (16 - d));
	return (((hi ^ pre[0]) & mh) | ((lo ^ pre[1]) & ml)) == 0;
}
// a digit on which all candidates agree is decided without a pass
__device__ __forceinline__ bool conv_uniform(const ConvHdr *h, int d)
{
	return conv_digit(h->any1[0] & h->any0[0], h->any1[1] & h->any0[1], d) == 0;
}

// Histogram of digit d over the candidates that match the digits decided so
// far: per-block bins in LDS, flushed once.  The high digits of a byte count
// are the same for nearly every candidate - 64 lanes on one LDS bin - so a
// wave first counts the lanes that share its first active lane's digit
// (ballot / popcount, one add) and only the others add for themselves.
__global__ __launch_bounds__(BLOCK) void conv_hist(ConvWs w, uint32_t k, int d)
{
	__shared__ uint32_t bins[256];
	const ConvHdr *h = w.h;
	const uint32_t n = conv_ncand(w);
	if (n <= k || conv_uniform(h, d) || (uint64_t)blockIdx.x * BLOCK >= n)
		return;   // (block-uniform)
	bins[threadIdx.x] = 0;
	__syncthreads();
	const uint64_t pre[2] = { h->pre[0], h->pre[1] };
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
#pragma unroll 1
	for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
		const uint64_t i = i0 + lane;
		bool act = false;
		uint32_t dg = 0;
		if (i < n) {
			const uint64_t hi = w.hi[i], lo = d > 7 ? w.lo[i] : 0;
			act = conv_above_match(hi, lo, pre, d);
			dg = conv_digit(hi, lo, d);
		}
		const uint64_t m = __ballot(act);
		if (!m)
			continue;
		const uint32_t lead = (uint32_t)__ffsll((long long)m) - 1;
		const uint32_t d0 = __shfl(dg, lead, 64);
		const uint64_t same = __ballot(act && dg == d0);
		if (lane == lead)
			atomicAdd(&bins[d0], (uint32_t)__popcll(same));
		else if (act && dg != d0)
			atomicAdd(&bins[dg], 1u);
	}
	__syncthreads();
	const uint32_t c = bins[threadIdx.x];
	if (c)
		(void)__hip_atomic_fetch_add(&w.h->bins[threadIdx.x], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave: the bin where the count from the top crosses the rows still
// wanted becomes digit d of the threshold; the bins are cleared for the next
// digit.  Lane l holds bins 4l .. 4l+3.
__global__ __launch_bounds__(64) void conv_scan(ConvWs w, uint32_t k, int d)
{
	ConvHdr *h = w.h;
	if (conv_ncand(w) <= k)
		return;
	const uint32_t lane = threadIdx.x;
	const uint32_t rem = d == 0 ? k : h->rem;
	const int shift = 8 * (7 - (d & 7));
	uint64_t *pre = &h->pre[d < 8 ? 0 : 1];
	if (conv_uniform(h, d)) {
		if (lane == 0) {
			*pre |= (uint64_t)conv_digit(h->any1[0], h->any1[1], d) << shift;
			h->rem = rem;
		}
		return;
	}
	uint4 *bp = (uint4 *)h->bins + lane;
	const uint4 b = *bp;
	const uint32_t mine = b.x + b.y + b.z + b.w;
	uint32_t v = mine;   // -> the sum over lanes >= this one
	for (uint32_t off = 1; off < 64; off <<= 1) {
		const uint32_t u = __shfl_down(v, off, 64);
		if (lane + off < 64)
			v += u;
	}
	uint32_t run = v - mine;   // candidates in bins above this lane's
	const uint32_t c[4] = { b.x, b.y, b.z, b.w };
	for (int j = 3; j >= 0; j--) {
		if (run < rem && rem - run <= c[j]) {
			*pre |= (uint64_t)(4 * lane + j) << shift;
			h->rem = rem - run;
		}
		run += c[j];
	}
	*bp = make_uint4(0, 0, 0, 0);
}

// Candidates above the threshold, and `rem` of those equal to it (more can tie
// only when bases were reused), write their row: positions 0 .. k - rem - 1
// and k - rem .. k - 1, each through a wave-aggregated cursor.  TS: nsd_convt
// rows, the smaller t_first and the larger t_last of the row's slot and `rev`.
template <bool TS>
__global__ __launch_bounds__(BLOCK) void conv_gather(Tab t, ConvWs w, uint32_t k, uint64_t *out, uint32_t *count)
{
	constexpr uint64_t ROW = TS ? 13 : 11;
	ConvHdr *h = w.h;
	const uint32_t n = conv_ncand(w);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		count[0] = n < k ? n : k;
		count[1] = n;
	}
	if (k == 0)
		return;
	const bool all = n <= k;
	const uint64_t th = h->pre[0], tl = h->pre[1];
	const uint32_t rem = all ? 0 : h->rem, base = all ? 0 : k - rem;
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK, below = (1ull << lane) - 1;
#pragma unroll 1
	for (uint64_t i0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
		const uint64_t i = i0 + lane;
		bool above = false, tied = false;
		if (i < n) {
			const uint64_t hi = w.hi[i], lo = w.lo[i];
			above = all || hi > th || (hi == th && lo > tl);
			tied = !all && hi == th && lo == tl;
		}
		const uint64_t ma = __ballot(above), mt = __ballot(tied);
		uint32_t a0 = 0, t0 = 0;
		if (lane == 0) {
			if (ma)
				a0 = __hip_atomic_fetch_add(&h->n_above, (uint32_t)__popcll(ma), __ATOMIC_RELAXED,
							    __HIP_MEMORY_SCOPE_AGENT);
			if (mt)
				t0 = __hip_atomic_fetch_add(&h->n_tied, (uint32_t)__popcll(mt), __ATOMIC_RELAXED,
							    __HIP_MEMORY_SCOPE_AGENT);
		}
		a0 = __shfl(a0, 0, 64);
		t0 = __shfl(t0, 0, 64);
		uint64_t pos = UINT64_MAX;
		if (above)
			pos = (uint64_t)a0 + (uint32_t)__popcll(ma & below);
		if (tied) {
			const uint64_t j = (uint64_t)t0 + (uint32_t)__popcll(mt & below);
			if (j < rem)
				pos = base + j;
		}
		if (pos >= k)
			continue;
		const uint32_t s = w.slot[i], r = w.rev[i];
		if (s >= t.slots || (r != NOSLOT && r >= t.slots))
			continue;
		const uint64_t *kp = t.key + 5ull * s;
		const Cnt c = t.cnt[s];
		Cnt e;
		e.pkts = e.bytes = e.last = 0;
		e.first = UINT64_MAX;
		e.flags = 0;
		if (r != NOSLOT)
			e = t.cnt[r];
		uint64_t *o = out + ROW * pos;
		o[0] = kp[0];
		o[1] = kp[1];
		o[2] = kp[2];
		o[3] = kp[3];
		o[4] = kp[4] | (uint64_t)(c.flags & 0xFFu) << 48 | (uint64_t)(e.flags & 0xFFu) << 56;
		o[5] = c.pkts;
		o[6] = c.bytes;
		o[7] = e.pkts;
		o[8] = e.bytes;
		o[9] = c.first < e.first ? c.first : e.first;
		o[10] = c.last > e.last ? c.last : e.last;
		if constexpr (TS) {
			uint64_t tf = t.tm[2ull * s], tl = t.tm[2ull * s + 1];
			if (r != NOSLOT) {
				const uint64_t rf = t.tm[2ull * r], rl = t.tm[2ull * r + 1];
				tf = rf < tf ? rf : tf;
				tl = rl > tl ? rl : tl;
			}
			o[11] = tf;
			o[12] = tl;
		}
	}
}

// ---- expiry -------------------------------------------------------------------
// Idle flows leave the table as rows (the header's "flow expiry").  Emptying a
// slot inside a probe chain would cut off every flow behind it - the next
// update would insert such a flow a second time - so nothing is deleted in
// place and the update / commit kernels know nothing of expiry: the table is
// rebuilt from its survivors.  After the commit on the table's stream, state is
// EMPTY or OCCUPIED:
//   expire_init      zeroes the workspace header (a kernel, as conv_init);
//   expire_split     reads the table: a qualifying flow takes a position from
//                    the `qualified` cursor and, below `max`, leaves as a row;
//                    every other flow copies its key and counters into the
//                    workspace through the `survivors` cursor;
//   expire_clear     nothing removed: returns, the table is not written at
//                    all.  Else every slot becomes what flow_reset makes it;
//   expire_reinsert  one survivor per lane claims the first EMPTY slot of its
//                    probe with one CAS EMPTY -> OCCUPIED and stores its rows.
// The flows removed are min(qualified, max): the positions below `max`.
//
// Workspace: an EXP_HDR-byte header, then the survivors' rows, 80 bytes each:
// the five key words, then the Cnt; on a timed table (TT) 96 bytes, the two
// times after them, whichever criterion the call uses.  The kernels bound the
// counts they read from the header by `slots`.
// BY_TIME (a timed table's nsd_flow_expire_device_ts): the criterion is t_last
// where it is `last` otherwise, and the rows that leave are nsd_flowt.
constexpr size_t EXP_HDR = 2048;
constexpr uint64_t exp_row_words(bool tt) { return tt ? 12 : 10; }

struct ExpHdr {
	uint32_t qualified;   // expire_split's cursor of qualifying flows
	uint32_t survivors;   // ... and of the flows that stay
	uint32_t lost;        // survivors that found no slot (cannot happen; the host entry checks)
	uint32_t pad;
};
static_assert(sizeof(ExpHdr) <= EXP_HDR, "expire header");

struct ExpWs {
	ExpHdr *h;
	uint64_t *rows;   // exp_row_words() per survivor
	uint32_t slots;
};

__global__ __launch_bounds__(BLOCK) void expire_init(ExpWs w)
{
	for (uint32_t i = threadIdx.x; i < EXP_HDR / 4; i += BLOCK)
		((uint32_t *)w.h)[i] = 0;
}

__device__ __forceinline__ uint32_t expire_removed(const ExpWs &w, uint32_t max)
{
	uint32_t n = w.h->qualified;
	n = n < w.slots ? n : w.slots;
	return n < max ? n : max;
}
__device__ __forceinline__ uint32_t expire_survivors(const ExpWs &w)
{
	const uint32_t n = w.h->survivors;
	return n < w.slots ? n : w.slots;
}

// a position for every lane of `m` from one atomic per wave (flow_export's cursor)
__device__ __forceinline__ uint64_t wave_cursor(uint32_t *cursor, uint64_t m, uint32_t lane)
{
	uint32_t at = 0;
	if (lane == 0)
		at = __hip_atomic_fetch_add(cursor, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	at = __shfl(at, 0, 64);
	return (uint64_t)at + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

// One slot per lane, grid-stride; only reads the table.
template <bool TT, bool BY_TIME>
__global__ __launch_bounds__(BLOCK) void expire_split(Tab t, ExpWs w, uint64_t before, uint32_t flags, uint64_t *out,
						      uint32_t max)
{
	static_assert(TT || !BY_TIME, "times only on a timed table");
	constexpr uint64_t ROW = BY_TIME ? 11 : 9, KEEP = exp_row_words(TT);
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
#pragma unroll 1
	for (uint64_t s0 = (uint64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u); s0 < t.slots; s0 += stride) {
		const uint64_t s = s0 + lane;
		const bool occ = s < t.slots && t.state[s] == OCCUPIED;
		if (!__ballot(occ))
			continue;
		Key k;
		Cnt c;
		bool idle = false;
		uint64_t tf = 0, tl = 0;
		if (occ) {
			load_key(t, (uint32_t)s, k);
			c = t.cnt[s];
			if constexpr (TT) {
				tf = t.tm[2 * s];
				tl = t.tm[2 * s + 1];
			}
			idle = (BY_TIME ? tl : c.last) < before;
			if (idle && (flags & NSD_FLOW_EXPIRE_PAIRED)) {
				Key r;
				reverse_key(k, r);
				if (!key_eq(k, r)) {
					const uint32_t rev = find_key(t, r);
					if (rev != NOSLOT)
						idle = (BY_TIME ? t.tm[2ull * rev + 1] : t.cnt[rev].last) < before;
				}
			}
		}
		const uint64_t mq = __ballot(idle);
		bool stay = occ && !idle;
		if (mq) {
			const uint64_t pos = wave_cursor(&w.h->qualified, mq, lane);
			if (idle) {
				if (pos < max) {
					uint64_t *o = out + ROW * pos;
					o[0] = k.w[0];
					o[1] = k.w[1];
					o[2] = k.w[2];
					o[3] = k.w[3];
					o[4] = k.w[4] | (uint64_t)(c.flags & 0xFFu) << 48;
					o[5] = c.pkts;
					o[6] = c.bytes;
					o[7] = c.first;
					o[8] = c.last;
					if constexpr (BY_TIME) {
						o[9] = tf;
						o[10] = tl;
					}
				} else {
					stay = true;   // no room for its row: it stays as it is
				}
			}
		}
		const uint64_t ms = __ballot(stay);
		if (!ms)
			continue;
		const uint64_t pos = wave_cursor(&w.h->survivors, ms, lane);
		// (max = 0 removes nothing: the rows would not be read)
		if (stay && max && pos < t.slots) {
			uint64_t *o = w.rows + KEEP * pos;
			o[0] = k.w[0];
			o[1] = k.w[1];
			o[2] = k.w[2];
			o[3] = k.w[3];
			o[4] = k.w[4];
			o[5] = c.pkts;
			o[6] = c.bytes;
			o[7] = c.first;
			o[8] = c.last;
			o[9] = c.flags;
			if constexpr (TT) {
				o[10] = tf;
				o[11] = tl;
			}
		}
	}
}

// count[0] = the flows removed, count[1] = those that qualified.  Nothing
// removed: the table stays as it is.  Else every slot as flow_reset leaves it;
// the stats stay but for FLOWS and EXPIRED.
__global__ __launch_bounds__(BLOCK) void expire_clear(Tab t, ExpWs w, uint32_t max, uint32_t *count)
{
	const uint32_t removed = expire_removed(w, max);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		count[0] = removed;
		count[1] = w.h->qualified;
		if (removed) {
			t.stats[NSD_FLOW_ST_FLOWS] -= removed;
			t.stats[NSD_FLOW_ST_EXPIRED] += removed;
		}
	}
	if (!removed)
		return;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.slots; s += stride)
		clear_slot(t, s);
}

// One survivor per lane, grid-stride.  Keys are unique, so a lane never
// compares against a slot: it takes the first EMPTY one of its probe (one
// relaxed CAS; a slot another lane took is passed by) and stores its own rows
// there with plain stores, which nobody reads before the next kernel.
template <bool TT>
__global__ __launch_bounds__(BLOCK) void expire_reinsert(Tab t, ExpWs w, uint32_t max)
{
	constexpr uint64_t KEEP = exp_row_words(TT);
	if (!expire_removed(w, max))
		return;
	const uint32_t n = expire_survivors(w);
	const uint32_t mask = t.slots - 1;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
#pragma unroll 1
	for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
		const uint64_t *r = w.rows + KEEP * i;
		Key k;
		for (int j = 0; j < 5; j++)
			k.w[j] = r[j];
		uint32_t s = (uint32_t)key_hash(k) & mask, slot = NOSLOT;
#pragma unroll 1
		for (uint32_t probes = 0; probes < t.slots; probes++, s = (s + 1) & mask) {
			if (__hip_atomic_load(&t.state[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != EMPTY)
				continue;
			uint32_t expect = EMPTY;
			if (__hip_atomic_compare_exchange_strong(&t.state[s], &expect, OCCUPIED, __ATOMIC_RELAXED,
								 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
				slot = s;
				break;
			}
		}
		if (slot == NOSLOT) {
			add_rlx(&w.h->lost, 1u);
			continue;
		}
		uint64_t *kp = t.key + 5ull * slot;
		for (int j = 0; j < 5; j++)
			kp[j] = k.w[j];
		Cnt c;
		c.pkts = r[5];
		c.bytes = r[6];
		c.first = r[7];
		c.last = r[8];
		c.flags = (uint32_t)r[9];
		c.pad = 0;
		t.cnt[slot] = c;
		if constexpr (TT) {
			t.tm[2ull * slot] = r[10];
			t.tm[2ull * slot + 1] = r[11];
		}
	}
}

// device staging of the host-memory entries (nsd_flow_batch, nsd_pcap_flows),
// grown on demand and kept with the table
struct Stage {
	uint8_t *frames = nullptr; size_t frames_cap = 0;
	uint64_t *desc = nullptr; size_t desc_cap = 0;
	uint64_t *desc_out = nullptr; size_t desc_out_cap = 0;
	uint32_t *verdict = nullptr; size_t verdict_cap = 0;
	nsd_rec *rec = nullptr; size_t rec_cap = 0;
	uint32_t *ext = nullptr; size_t ext_cap = 0;
	uint8_t *ws = nullptr; size_t ws_cap = 0;
	uint8_t *bpf_ws = nullptr; size_t bpf_ws_cap = 0;
	nsd_sll_t *sll = nullptr; size_t sll_cap = 0;
	uint8_t *misc = nullptr; size_t misc_cap = 0;   // ext_used | count | counters
	uint64_t *ts = nullptr; size_t ts_cap = 0;      // (a timed table's feeds)

	void release()
	{
		(void)hipFree(frames); (void)hipFree(desc); (void)hipFree(desc_out); (void)hipFree(verdict);
		(void)hipFree(rec); (void)hipFree(ext); (void)hipFree(ws); (void)hipFree(bpf_ws); (void)hipFree(sll);
		(void)hipFree(misc); (void)hipFree(ts);
		*this = Stage();
	}
};

} // namespace nsdflow

using namespace nsdflow;

struct nsd_flow_table {
	Tab tab{};
	void *mem = nullptr;
	bool timed = false;   // tab.tm is there: the _ts entries, and no plain update
	int cus = 0;
	hipStream_t last = nullptr;   // the stream of the last enqueued call
	Stage stage;
};

static int grid_for(const nsd_flow_table *t, uint64_t items)
{
	const uint64_t blocks = (items + BLOCK - 1) / BLOCK;
	const uint64_t cap = (uint64_t)(t->cus > 0 ? t->cus : 256) * 8;
	return (int)(blocks < cap ? (blocks ? blocks : 1) : cap);
}

extern "C" uint32_t nsd_flow_slots(const nsd_flow_table *t) { return t ? t->tab.slots : 0; }

extern "C" int nsd_flow_reset(nsd_flow_table *t, void *stream)
{
	if (!t)
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(flow_reset, dim3(grid_for(t, t->tab.slots)), dim3(BLOCK), 0, s, t->tab);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

extern "C" int nsd_flow_is_timed(const nsd_flow_table *t) { return t && t->timed; }

static nsd_flow_table *create_table(uint32_t max_flows, bool timed)
{
	if (max_flows == 0 || max_flows > (1u << 30))
		return nullptr;
	int ndev = 0, dev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
		fprintf(stderr, "netsniff-dissect flow: no GPU\n");
		return nullptr;
	}
	uint32_t slots = 2;
	while (slots < 2ull * max_flows)
		slots <<= 1;
	nsd_flow_table *t = new (std::nothrow) nsd_flow_table;
	if (!t)
		return nullptr;
	hipDeviceProp_t prop;
	if (hip_ok(hipGetDevice(&dev), "hipGetDevice") && hip_ok(hipGetDeviceProperties(&prop, dev), "props"))
		t->cus = prop.multiProcessorCount;
	// one allocation: state | stats | key | cnt, and behind them a timed table's tm
	const size_t a = 256;
	auto up = [&](size_t v) { return (v + a - 1) & ~(a - 1); };
	const size_t o_state = 0, o_misc = up((size_t)slots * 4), o_key = o_misc + a, o_cnt = o_key + up((size_t)slots * 40), total = o_cnt + up((size_t)slots * 40);
	if (!hip_ok(hipMalloc(&t->mem, total + (timed ? (size_t)slots * 16 : 0)), "hipMalloc")) {
		delete t;
		return nullptr;
	}
	uint8_t *m = (uint8_t *)t->mem;
	t->tab.state = (uint32_t *)(m + o_state);
	t->tab.stats = (uint64_t *)(m + o_misc);
	t->tab.key = (uint64_t *)(m + o_key);
	t->tab.cnt = (Cnt *)(m + o_cnt);
	t->tab.slots = slots;
	t->tab.tm = timed ? (uint64_t *)(m + total) : nullptr;
	t->timed = timed;
	if (nsd_flow_reset(t, nullptr) != NSD_OK || !hip_ok(hipStreamSynchronize(nullptr), "sync")) {
		(void)hipFree(t->mem);
		delete t;
		return nullptr;
	}
	return t;
}

extern "C" nsd_flow_table *nsd_flow_create(uint32_t max_flows) { return create_table(max_flows, false); }
extern "C" nsd_flow_table *nsd_flow_create_timed(uint32_t max_flows) { return create_table(max_flows, true); }

extern "C" void nsd_flow_destroy(nsd_flow_table *t)
{
	if (!t)
		return;
	(void)hipDeviceSynchronize();
	t->stage.release();
	(void)hipFree(t->mem);
	delete t;
}

// The entries come in two forms, the plain one and the _ts one with the times
// (the header's "flow times"); each pair shares its body.  `ts` = the _ts form
// was called: on a plain table that is NSD_ERR_ARG, and so is the plain update
// on a timed table (its flows would be left without times).
template <class Row>
constexpr bool with_times()
{
	return std::is_same<Row, nsd_flowt>::value || std::is_same<Row, nsd_convt>::value;
}

static int update_device(nsd_flow_table *t, const uint8_t *d_frames, const nsd_desc_t *d_desc, uint32_t n,
			 const nsd_rec *d_rec, const uint32_t *d_ext, uint32_t ext_words, const uint64_t *d_ts, bool ts,
			 uint64_t base, void *stream)
{
	if (!t || n > MAX_N || ts != t->timed)
		return NSD_ERR_ARG;
	if (n == 0)
		return NSD_OK;
	if (!d_frames || !d_desc || !d_rec || (ext_words && !d_ext) || (ts && !d_ts))
		return NSD_ERR_ARG;
	if (((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ext & 3) || ((uintptr_t)d_ts & 7))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const In in{ d_frames, (const uint64_t *)d_desc, d_rec, ext_words ? d_ext : nullptr, ext_words, n, base,
		     ts ? d_ts : nullptr };
	const dim3 grid(grid_for(t, n)), block(BLOCK);
	if (ts)
		hipLaunchKernelGGL(flow_update<true>, grid, block, 0, s, t->tab, in);
	else
		hipLaunchKernelGGL(flow_update<false>, grid, block, 0, s, t->tab, in);
	hipLaunchKernelGGL(flow_commit, dim3(grid_for(t, t->tab.slots)), block, 0, s, t->tab, in);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

extern "C" int nsd_flow_update_device(nsd_flow_table *t, const uint8_t *d_frames, const nsd_desc_t *d_desc,
				      uint32_t n, const nsd_rec *d_rec, const uint32_t *d_ext, uint32_t ext_words,
				      uint64_t base, void *stream)
{
	return update_device(t, d_frames, d_desc, n, d_rec, d_ext, ext_words, nullptr, false, base, stream);
}

extern "C" int nsd_flow_update_device_ts(nsd_flow_table *t, const uint8_t *d_frames, const nsd_desc_t *d_desc,
					 uint32_t n, const nsd_rec *d_rec, const uint32_t *d_ext, uint32_t ext_words,
					 const uint64_t *d_ts, uint64_t base, void *stream)
{
	return update_device(t, d_frames, d_desc, n, d_rec, d_ext, ext_words, d_ts, true, base, stream);
}

static int export_device(nsd_flow_table *t, void *d_flows, uint32_t max, uint32_t *d_count, uint64_t *d_stats,
			 void *stream, bool ts)
{
	if (!t || (ts && !t->timed) || !d_count || !d_stats || (max && !d_flows) || ((uintptr_t)d_flows & 7))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	if (!hip_ok(hipMemsetAsync(d_count, 0, 4, s), "memset"))
		return NSD_ERR_HIP;
	const dim3 grid(grid_for(t, t->tab.slots)), block(BLOCK);
	if (ts)
		hipLaunchKernelGGL(flow_export<true>, grid, block, 0, s, t->tab, (uint64_t *)d_flows, max, d_count, d_stats);
	else
		hipLaunchKernelGGL(flow_export<false>, grid, block, 0, s, t->tab, (uint64_t *)d_flows, max, d_count, d_stats);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

extern "C" int nsd_flow_export_device(nsd_flow_table *t, nsd_flow *d_flows, uint32_t max, uint32_t *d_count,
				      uint64_t *d_stats, void *stream)
{
	return export_device(t, d_flows, max, d_count, d_stats, stream, false);
}

extern "C" int nsd_flow_export_device_ts(nsd_flow_table *t, nsd_flowt *d_flows, uint32_t max, uint32_t *d_count,
					 uint64_t *d_stats, void *stream)
{
	return export_device(t, d_flows, max, d_count, d_stats, stream, true);
}

template <class Row>
static void sort_by_first(std::vector<Row> &v)
{
	std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) { return a.first < b.first; });
}

template <class Row>
static long export_host(nsd_flow_table *t, Row *flows, uint32_t max, uint64_t *stats)
{
	if (!t || (with_times<Row>() && !t->timed) || (max && !flows))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") ||
	    !hip_ok(hipStreamSynchronize(s), "sync"))
		return NSD_ERR_HIP;
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS];
	uint8_t *d = nullptr;
	if (!hip_ok(hipMalloc(&d, 256 + (size_t)have * sizeof(Row)), "hipMalloc"))
		return NSD_ERR_NOMEM;
	uint32_t *d_count = (uint32_t *)d;
	uint64_t *d_stats = (uint64_t *)(d + 64);
	Row *d_flows = (Row *)(d + 256);
	std::vector<Row> rows(have);
	uint32_t count = 0;
	bool ok = export_device(t, d_flows, have, d_count, d_stats, s, with_times<Row>()) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") &&
		  (!have || hip_ok(hipMemcpyAsync(rows.data(), d_flows, (size_t)have * sizeof(Row),
						  hipMemcpyDeviceToHost, s), "D2H")) &&
		  hip_ok(hipStreamSynchronize(s), "sync");
	(void)hipFree(d);
	if (!ok || count != have)
		return NSD_ERR_HIP;
	sort_by_first(rows);
	const uint32_t k = have < max ? have : max;
	if (k)
		memcpy(flows, rows.data(), (size_t)k * sizeof(Row));
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)have;
}

extern "C" long nsd_flow_export(nsd_flow_table *t, nsd_flow *flows, uint32_t max, uint64_t *stats)
{
	return export_host(t, flows, max, stats);
}

extern "C" long nsd_flow_export_ts(nsd_flow_table *t, nsd_flowt *flows, uint32_t max, uint64_t *stats)
{
	return export_host(t, flows, max, stats);
}

// ---- conversations: the entries ---------------------------------------------
static_assert(sizeof(nsd_conv) == 88 && offsetof(nsd_conv, pkts_src) == 40, "nsd_conv");

extern "C" size_t nsd_flow_conv_workspace_bytes(const nsd_flow_table *t)
{
	return t ? CONV_HDR + 24 * (size_t)t->tab.slots : 0;
}

// init | pair | per digit: hist, scan | gather: a linear chain of kernels on `stream`
static int conv_device(nsd_flow_table *t, int by, uint32_t k, void *d_conv, uint32_t *d_count, void *d_workspace,
		       void *stream, bool ts)
{
	if (!t || (ts && !t->timed) || by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || !d_count || !d_workspace ||
	    (k && !d_conv) || ((uintptr_t)d_conv & 7) || ((uintptr_t)d_workspace & 15) || ((uintptr_t)d_count & 3))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const size_t slots = t->tab.slots;
	uint8_t *m = (uint8_t *)d_workspace;
	ConvWs w;
	w.h = (ConvHdr *)m;
	w.hi = (uint64_t *)(m + CONV_HDR);
	w.lo = w.hi + slots;
	w.slot = (uint32_t *)(w.lo + slots);
	w.rev = w.slot + slots;
	w.slots = t->tab.slots;
	const dim3 grid(grid_for(t, slots)), block(BLOCK);
	hipLaunchKernelGGL(conv_init, dim3(1), block, 0, s, w);
	hipLaunchKernelGGL(conv_pair, grid, block, 0, s, t->tab, w, by);
	if (k && k < slots) {   // (k >= slots: every conversation is wanted)
		const int digits = by == NSD_CONV_BY_FIRST ? CONV_DIGITS / 2 : CONV_DIGITS;
		for (int d = 0; d < digits; d++) {
			hipLaunchKernelGGL(conv_hist, grid, block, 0, s, w, k, d);
			hipLaunchKernelGGL(conv_scan, dim3(1), dim3(64), 0, s, w, k, d);
		}
	}
	if (ts)
		hipLaunchKernelGGL(conv_gather<true>, grid, block, 0, s, t->tab, w, k, (uint64_t *)d_conv, d_count);
	else
		hipLaunchKernelGGL(conv_gather<false>, grid, block, 0, s, t->tab, w, k, (uint64_t *)d_conv, d_count);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

extern "C" int nsd_flow_conv_device(nsd_flow_table *t, int by, uint32_t k, nsd_conv *d_conv, uint32_t *d_count,
				    void *d_workspace, void *stream)
{
	return conv_device(t, by, k, d_conv, d_count, d_workspace, stream, false);
}

extern "C" int nsd_flow_conv_device_ts(nsd_flow_table *t, int by, uint32_t k, nsd_convt *d_conv, uint32_t *d_count,
				       void *d_workspace, void *stream)
{
	return conv_device(t, by, k, d_conv, d_count, d_workspace, stream, true);
}

// the total order of the header: `by`'s metric descending, then first ascending
template <class Conv>
static void sort_conv(std::vector<Conv> &v, int by)
{
	std::sort(v.begin(), v.end(), [by](const Conv &a, const Conv &b) {
		if (by != NSD_CONV_BY_FIRST) {
			const uint64_t ma = by == NSD_CONV_BY_BYTES ? a.bytes_src + a.bytes_dst : a.pkts_src + a.pkts_dst;
			const uint64_t mb = by == NSD_CONV_BY_BYTES ? b.bytes_src + b.bytes_dst : b.pkts_src + b.pkts_dst;
			if (ma != mb)
				return ma > mb;
		}
		return a.first < b.first;
	});
}

template <class Conv>
static long conversations_host(nsd_flow_table *t, int by, uint32_t k, Conv *conv, uint64_t *stats)
{
	if (!t || (with_times<Conv>() && !t->timed) || by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || (k && !conv))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") ||
	    !hip_ok(hipStreamSynchronize(s), "sync"))
		return NSD_ERR_HIP;
	// (no more conversations than flows)
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS], want = k < have ? k : have;
	const size_t o_rows = 256, o_ws = (o_rows + (size_t)want * sizeof(Conv) + 255) & ~(size_t)255;
	uint8_t *d = nullptr;
	if (!hip_ok(hipMalloc(&d, o_ws + nsd_flow_conv_workspace_bytes(t)), "hipMalloc"))
		return NSD_ERR_NOMEM;
	uint32_t *d_count = (uint32_t *)d;
	Conv *d_rows = (Conv *)(d + o_rows);
	uint32_t count[2] = { 0, 0 };
	std::vector<Conv> rows;
	bool ok = conv_device(t, by, want, d_rows, d_count, d + o_ws, s, with_times<Conv>()) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(count, d_count, 8, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipStreamSynchronize(s), "sync") && count[0] <= want;
	if (ok && count[0]) {
		rows.resize(count[0]);
		ok = hip_ok(hipMemcpy(rows.data(), d_rows, (size_t)count[0] * sizeof(Conv), hipMemcpyDeviceToHost), "D2H");
	}
	(void)hipFree(d);
	if (!ok)
		return NSD_ERR_HIP;
	sort_conv(rows, by);
	if (!rows.empty())
		memcpy(conv, rows.data(), rows.size() * sizeof(Conv));
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)count[1];
}

extern "C" long nsd_flow_conversations(nsd_flow_table *t, int by, uint32_t k, nsd_conv *conv, uint64_t *stats)
{
	return conversations_host(t, by, k, conv, stats);
}

extern "C" long nsd_flow_conversations_ts(nsd_flow_table *t, int by, uint32_t k, nsd_convt *conv, uint64_t *stats)
{
	return conversations_host(t, by, k, conv, stats);
}

// ---- expiry: the entries ------------------------------------------------------
extern "C" size_t nsd_flow_expire_workspace_bytes(const nsd_flow_table *t)
{
	return t ? EXP_HDR + 8 * exp_row_words(t->timed) * (size_t)t->tab.slots : 0;
}

// init | split | clear | reinsert: a linear chain of kernels on `stream`.  A
// timed table's survivors carry their times through the workspace under
// either criterion.
static int expire_device(nsd_flow_table *t, uint64_t before, uint32_t flags, void *d_expired, uint32_t max,
			 uint32_t *d_count, void *d_workspace, void *stream, bool ts)
{
	if (!t || (ts && !t->timed) || (flags & ~NSD_FLOW_EXPIRE_PAIRED) || !d_count || !d_workspace ||
	    (max && !d_expired) || ((uintptr_t)d_expired & 7) || ((uintptr_t)d_workspace & 15) || ((uintptr_t)d_count & 3))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	uint8_t *m = (uint8_t *)d_workspace;
	const ExpWs w{ (ExpHdr *)m, (uint64_t *)(m + EXP_HDR), t->tab.slots };
	const dim3 grid(grid_for(t, t->tab.slots)), block(BLOCK);
	uint64_t *out = (uint64_t *)d_expired;
	hipLaunchKernelGGL(expire_init, dim3(1), block, 0, s, w);
	if (ts)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(expire_split<true, true>), grid, block, 0, s, t->tab, w, before, flags, out,
				   max);
	else if (t->timed)
		hipLaunchKernelGGL(HIP_KERNEL_NAME(expire_split<true, false>), grid, block, 0, s, t->tab, w, before, flags, out,
				   max);
	else
		hipLaunchKernelGGL(HIP_KERNEL_NAME(expire_split<false, false>), grid, block, 0, s, t->tab, w, before, flags,
				   out, max);
	hipLaunchKernelGGL(expire_clear, grid, block, 0, s, t->tab, w, max, d_count);
	if (t->timed)
		hipLaunchKernelGGL(expire_reinsert<true>, grid, block, 0, s, t->tab, w, max);
	else
		hipLaunchKernelGGL(expire_reinsert<false>, grid, block, 0, s, t->tab, w, max);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

extern "C" int nsd_flow_expire_device(nsd_flow_table *t, uint64_t before, uint32_t flags, nsd_flow *d_expired,
				      uint32_t max, uint32_t *d_count, void *d_workspace, void *stream)
{
	return expire_device(t, before, flags, d_expired, max, d_count, d_workspace, stream, false);
}

extern "C" int nsd_flow_expire_device_ts(nsd_flow_table *t, uint64_t before_ns, uint32_t flags, nsd_flowt *d_expired,
					 uint32_t max, uint32_t *d_count, void *d_workspace, void *stream)
{
	return expire_device(t, before_ns, flags, d_expired, max, d_count, d_workspace, stream, true);
}

template <class Row>
static long expire_rows(nsd_flow_table *t, uint64_t before, uint32_t flags, uint32_t max, std::vector<Row> &rows,
			uint64_t *stats)
{
	rows.clear();
	if (!t || (with_times<Row>() && !t->timed) || (flags & ~NSD_FLOW_EXPIRE_PAIRED))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") ||
	    !hip_ok(hipStreamSynchronize(s), "sync"))
		return NSD_ERR_HIP;
	// (no more rows than flows)
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS], want = max < have ? max : have;
	const size_t o_rows = 256, o_ws = (o_rows + (size_t)want * sizeof(Row) + 255) & ~(size_t)255;
	uint8_t *d = nullptr;
	if (!hip_ok(hipMalloc(&d, o_ws + nsd_flow_expire_workspace_bytes(t)), "hipMalloc"))
		return NSD_ERR_NOMEM;
	uint32_t *d_count = (uint32_t *)d;
	Row *d_rows = (Row *)(d + o_rows);
	uint32_t count[2] = { 0, 0 };
	ExpHdr h{};
	bool ok = expire_device(t, before, flags, d_rows, want, d_count, d + o_ws, s, with_times<Row>()) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(count, d_count, 8, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(&h, d + o_ws, sizeof(h), hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipStreamSynchronize(s), "sync") && count[0] <= want;
	if (ok && count[0]) {
		rows.resize(count[0]);
		ok = hip_ok(hipMemcpy(rows.data(), d_rows, (size_t)count[0] * sizeof(Row), hipMemcpyDeviceToHost), "D2H");
	}
	(void)hipFree(d);
	// every flow of before either left as a row or is back in the table
	if (!ok || h.lost || (uint64_t)count[0] + h.survivors != have || st[NSD_FLOW_ST_FLOWS] != h.survivors) {
		rows.clear();
		return NSD_ERR_HIP;
	}
	sort_by_first(rows);
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)count[1];
}

long nsd_flow_expire_rows(nsd_flow_table *t, uint64_t before, uint32_t flags, uint32_t max,
			  std::vector<nsd_flow> &rows, uint64_t *stats)
{
	return expire_rows(t, before, flags, max, rows, stats);
}

long nsd_flow_expire_rows_ts(nsd_flow_table *t, uint64_t before_ns, uint32_t flags, uint32_t max,
			     std::vector<nsd_flowt> &rows, uint64_t *stats)
{
	return expire_rows(t, before_ns, flags, max, rows, stats);
}

template <class Row>
static long expire_host(nsd_flow_table *t, uint64_t before, uint32_t flags, Row *expired, uint32_t max, uint64_t *stats)
{
	if (max && !expired)
		return NSD_ERR_ARG;
	std::vector<Row> rows;
	const long q = expire_rows(t, before, flags, max, rows, stats);
	if (q >= 0 && !rows.empty())
		memcpy(expired, rows.data(), rows.size() * sizeof(Row));
	return q;
}

extern "C" long nsd_flow_expire(nsd_flow_table *t, uint64_t before, uint32_t flags, nsd_flow *expired, uint32_t max,
				uint64_t *stats)
{
	return expire_host(t, before, flags, expired, max, stats);
}

extern "C" long nsd_flow_expire_ts(nsd_flow_table *t, uint64_t before_ns, uint32_t flags, nsd_flowt *expired,
				   uint32_t max, uint64_t *stats)
{
	return expire_host(t, before_ns, flags, expired, max, stats);
}

// ---- the same aggregation on the host -----------------------------------
namespace {
struct KeyHash {
	size_t operator()(const Key &k) const { return (size_t)key_hash(k); }
};
struct KeyEq {
	bool operator()(const Key &a, const Key &b) const { return key_eq(a, b); }
};
// the key bytes of a row (either row type begins with them)
template <class Row>
Key key_of(const Row &f)
{
	Key k;
	memcpy(k.w, &f, 40);
	k.w[4] &= 0x0000FFFFFFFFFFFFull;   // tcp_flags, rsvd
	return k;
}
// the row of the reverse key: src / dst and sport / dport swapped
template <class Row>
Key reverse_of(const Row &f)
{
	Row r = f;
	memcpy(r.src, f.dst, 16);
	memcpy(r.dst, f.src, 16);
	r.sport = f.dport;
	r.dport = f.sport;
	return key_of(r);
}
// what expires a row: its t_last where the rows carry times, else its `last`
inline uint64_t idle_mark(const nsd_flow &f) { return f.last; }
inline uint64_t idle_mark(const nsd_flowt &f) { return f.t_last; }
} // namespace

// Row = nsd_flowt: ts[n], and each row's t_first / t_last = the smallest /
// largest timestamp of its packets.
template <class Row>
static long flow_cpu(const uint8_t *frames, const nsd_desc_t *desc, uint32_t n, const nsd_rec *rec, const uint32_t *ext,
		     const uint64_t *ts, uint64_t base, Row *flows, uint32_t max, uint64_t *stats)
{
	if (n > MAX_N || (n && (!frames || !desc || !rec || (with_times<Row>() && !ts))) || (max && !flows))
		return NSD_ERR_ARG;
	std::unordered_map<Key, Row, KeyHash, KeyEq> map;
	uint64_t st[NSD_FLOW_NSTATS] = { 0 };
	for (uint32_t i = 0; i < n; i++) {
		Key k;
		uint32_t tf = 0;
		const uint32_t caplen = NSD_DESC_CAPLEN(desc[i]);
		const int r = flow_key(rec[i], ext, ext ? UINT32_MAX : 0, frames + NSD_DESC_OFF(desc[i]), caplen, k, tf);
		st[NSD_FLOW_ST_PKTS]++;
		if (r != K_KEYED) {
			st[r == K_NOIP ? NSD_FLOW_ST_NOIP : NSD_FLOW_ST_SKIPPED]++;
			continue;
		}
		st[NSD_FLOW_ST_KEYED]++;
		auto it = map.find(k);
		if (it == map.end()) {
			Row f;
			memset(&f, 0, sizeof(f));
			memcpy(&f, k.w, 40);
			f.first = base + i;
			if constexpr (with_times<Row>())
				f.t_first = UINT64_MAX;
			it = map.emplace(k, f).first;
		}
		Row &f = it->second;
		f.pkts++;
		f.bytes += caplen;
		f.last = base + i;
		f.tcp_flags |= (uint8_t)tf;
		if constexpr (with_times<Row>()) {
			f.t_first = ts[i] < f.t_first ? ts[i] : f.t_first;
			f.t_last = ts[i] > f.t_last ? ts[i] : f.t_last;
		}
	}
	st[NSD_FLOW_ST_FLOWS] = map.size();
	std::vector<Row> rows;
	rows.reserve(map.size());
	for (const auto &kv : map)
		rows.push_back(kv.second);
	sort_by_first(rows);
	const size_t k = rows.size() < max ? rows.size() : max;
	if (k)
		memcpy(flows, rows.data(), k * sizeof(Row));
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)rows.size();
}

extern "C" long nsd_flow_cpu(const uint8_t *frames, const nsd_desc_t *desc, uint32_t n, const nsd_rec *rec,
			     const uint32_t *ext, uint64_t base, nsd_flow *flows, uint32_t max, uint64_t *stats)
{
	return flow_cpu(frames, desc, n, rec, ext, nullptr, base, flows, max, stats);
}

extern "C" long nsd_flow_cpu_ts(const uint8_t *frames, const nsd_desc_t *desc, uint32_t n, const nsd_rec *rec,
				const uint32_t *ext, const uint64_t *ts, uint64_t base, nsd_flowt *flows, uint32_t max,
				uint64_t *stats)
{
	return flow_cpu(frames, desc, n, rec, ext, ts, base, flows, max, stats);
}

// Flow rows (unique keys, any order) paired into conversations on the host:
// a hash map from key to row, one lookup of the reverse per row.  Rows with
// times give conversations with times: min / max over both directions.
template <class Row, class Conv>
static long conv_cpu(const Row *flows, size_t n, int by, Conv *conv, uint32_t max)
{
	static_assert(with_times<Row>() == with_times<Conv>(), "rows and conversations of one kind");
	if (by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || (n && !flows) || (max && !conv))
		return NSD_ERR_ARG;
	std::unordered_map<Key, size_t, KeyHash, KeyEq> map;
	map.reserve(n);
	for (size_t i = 0; i < n; i++)
		map.emplace(key_of(flows[i]), i);
	std::vector<Conv> rows;
	for (size_t i = 0; i < n; i++) {
		const Row &f = flows[i];
		const Key k = key_of(f), kr = reverse_of(f);
		const auto it = key_eq(k, kr) ? map.end() : map.find(kr);
		const Row *g = it == map.end() ? nullptr : &flows[it->second];
		if (g && (g->first < f.first || (g->first == f.first && memcmp(kr.w, k.w, 40) < 0)))
			continue;   // the reverse is the originator: its row carries this one
		Conv c;
		memset(&c, 0, sizeof(c));
		memcpy(&c, k.w, 40);
		c.tcp_flags_src = f.tcp_flags;
		c.pkts_src = f.pkts;
		c.bytes_src = f.bytes;
		c.first = f.first;
		c.last = f.last;
		if constexpr (with_times<Row>()) {
			c.t_first = f.t_first;
			c.t_last = f.t_last;
		}
		if (g) {
			c.tcp_flags_dst = g->tcp_flags;
			c.pkts_dst = g->pkts;
			c.bytes_dst = g->bytes;
			c.last = g->last > f.last ? g->last : f.last;
			if constexpr (with_times<Row>()) {
				c.t_first = g->t_first < f.t_first ? g->t_first : f.t_first;
				c.t_last = g->t_last > f.t_last ? g->t_last : f.t_last;
			}
		}
		rows.push_back(c);
	}
	sort_conv(rows, by);
	const size_t k = rows.size() < max ? rows.size() : max;
	if (k)
		memcpy(conv, rows.data(), k * sizeof(Conv));
	return (long)rows.size();
}

extern "C" long nsd_conv_cpu(const nsd_flow *flows, size_t n, int by, nsd_conv *conv, uint32_t max)
{
	return conv_cpu(flows, n, by, conv, max);
}

extern "C" long nsd_conv_cpu_ts(const nsd_flowt *flows, size_t n, int by, nsd_convt *conv, uint32_t max)
{
	return conv_cpu(flows, n, by, conv, max);
}

// The expiry rules on the host over flow rows (unique keys, any order): a hash
// map from key to row for the reverse lookup.  Survivors keep their input
// order at the front of `flows`; the first `max` qualifying rows in input
// order go to `expired`, the others stay.  Rows with times expire by t_last
// (idle_mark).
template <class Row>
static long expire_cpu(Row *flows, size_t n, uint64_t before, uint32_t flags, Row *expired, uint32_t max,
		       size_t *remaining)
{
	if ((flags & ~NSD_FLOW_EXPIRE_PAIRED) || (n && !flows) || (max && !expired) || !remaining)
		return NSD_ERR_ARG;
	std::unordered_map<Key, size_t, KeyHash, KeyEq> map;
	if (flags & NSD_FLOW_EXPIRE_PAIRED) {
		map.reserve(n);
		for (size_t i = 0; i < n; i++)
			map.emplace(key_of(flows[i]), i);
	}
	// decided over the rows as given, before any of them moves
	std::vector<uint8_t> idle(n);
	for (size_t i = 0; i < n; i++) {
		const Row &f = flows[i];
		idle[i] = idle_mark(f) < before;
		if (!idle[i] || !(flags & NSD_FLOW_EXPIRE_PAIRED))
			continue;
		const Key k = key_of(f), kr = reverse_of(f);
		const auto it = key_eq(k, kr) ? map.end() : map.find(kr);
		if (it != map.end())
			idle[i] = idle_mark(flows[it->second]) < before;
	}
	size_t qualified = 0, kept = 0;
	for (size_t i = 0; i < n; i++) {
		if (idle[i] && qualified++ < max)
			expired[qualified - 1] = flows[i];
		else
			flows[kept++] = flows[i];
	}
	*remaining = kept;
	return (long)qualified;
}

extern "C" long nsd_flow_expire_cpu(nsd_flow *flows, size_t n, uint64_t before, uint32_t flags, nsd_flow *expired,
				    uint32_t max, size_t *remaining)
{
	return expire_cpu(flows, n, before, flags, expired, max, remaining);
}

extern "C" long nsd_flow_expire_cpu_ts(nsd_flowt *flows, size_t n, uint64_t before_ns, uint32_t flags,
				       nsd_flowt *expired, uint32_t max, size_t *remaining)
{
	return expire_cpu(flows, n, before_ns, flags, expired, max, remaining);
}

// ---- host-memory entries --------------------------------------------------
// Records made on the host (a record no batch carries, walked by the
// per-packet path) into the table: n packets of `frames` with their records
// and ext pool; ts[n] = their timestamps, for a timed table (else ignored).
// Synchronous.
extern "C" __attribute__((visibility("hidden"))) int nsd_flow_feed_records(nsd_flow_table *t, const uint8_t *frames,
									    size_t frames_len, const nsd_desc_t *desc,
									    uint32_t n, const nsd_rec *rec,
									    const uint32_t *ext, uint32_t ext_words,
									    const uint64_t *ts, uint64_t base)
{
	if (!t || !n)
		return t ? NSD_OK : NSD_ERR_ARG;
	if (t->timed && !ts)
		return NSD_ERR_ARG;
	Stage &g = t->stage;
	hipStream_t s = t->last;
	if (!grow(g.frames, g.frames_cap, frames_len + NSD_FRAME_PAD) || !grow(g.desc, g.desc_cap, n) ||
	    !grow(g.rec, g.rec_cap, n) || (ext_words && !grow(g.ext, g.ext_cap, ext_words)) ||
	    (t->timed && !grow(g.ts, g.ts_cap, n)))
		return NSD_ERR_NOMEM;
	bool ok = hip_ok(hipMemcpyAsync(g.frames, frames, frames_len, hipMemcpyHostToDevice, s), "H2D") &&
		  hip_ok(hipMemsetAsync(g.frames + frames_len, 0, NSD_FRAME_PAD, s), "memset") &&
		  hip_ok(hipMemcpyAsync(g.desc, desc, (size_t)n * 8, hipMemcpyHostToDevice, s), "H2D") &&
		  hip_ok(hipMemcpyAsync(g.rec, rec, (size_t)n * sizeof(nsd_rec), hipMemcpyHostToDevice, s), "H2D") &&
		  (!ext_words || hip_ok(hipMemcpyAsync(g.ext, ext, (size_t)ext_words * 4, hipMemcpyHostToDevice, s), "H2D")) &&
		  (!t->timed || hip_ok(hipMemcpyAsync(g.ts, ts, (size_t)n * 8, hipMemcpyHostToDevice, s), "H2D"));
	if (!ok)
		return NSD_ERR_HIP;
	const int rc = update_device(t, g.frames, g.desc, n, g.rec, g.ext, ext_words, g.ts, t->timed, base, s);
	if (rc != NSD_OK)
		return rc;
	return hip_ok(hipStreamSynchronize(s), "sync") ? NSD_OK : NSD_ERR_HIP;
}

// A host-memory batch into the table: staged, filtered by the optional BPF
// program (accepted descriptors packed on the device, nsd_bpf_filter_device),
// walked and accumulated, in chunks whose ext pool stays small.  The packets
// fed get base, base + 1, ...  Returns their number or a negative NSD_ERR_*.
// A timed table takes ts[n], the packets' timestamps (else ignored): those of
// the accepted packets are packed on the host by the verdicts, as the sll
// entries are, and *ts_max (may be NULL) is raised to the largest one fed.
// Synchronous.
extern "C" __attribute__((visibility("hidden"))) long nsd_flow_feed_host(nsd_flow_table *t, const uint8_t *frames,
									  size_t frames_len, const nsd_desc_t *desc,
									  const nsd_sll_t *sll, uint32_t n, int linktype,
									  int mode, const nsd_bpf_prog *filter, const uint64_t *ts,
									  uint64_t *ts_max, uint64_t base)
{
	if (!t || mode < PRINT_NORM || mode > PRINT_NONE || (n && (!frames || !desc || (t->timed && !ts))))
		return NSD_ERR_ARG;
	if (!t->timed)
		ts = nullptr;
	if (n == 0)
		return 0;
	for (uint32_t i = 0; i < n; i++) {
		if (NSD_DESC_CAPLEN(desc[i]) > NSD_MAX_CAPLEN)
			return NSD_ERR_CAPLEN;
		if (NSD_DESC_OFF(desc[i]) + NSD_DESC_CAPLEN(desc[i]) > frames_len)
			return NSD_ERR_ARG;
	}
	constexpr uint32_t CHUNK = 1u << 18;
	Stage &g = t->stage;
	hipStream_t s = t->last;
	const uint32_t most = n < CHUNK ? n : CHUNK;
	const uint32_t ext_words = (uint32_t)NSD_EXT_POOL_WORDS(most);
	if (!grow(g.frames, g.frames_cap, frames_len + NSD_FRAME_PAD) || !grow(g.desc, g.desc_cap, most) ||
	    !grow(g.rec, g.rec_cap, most) || !grow(g.ext, g.ext_cap, ext_words) ||
	    !grow(g.ws, g.ws_cap, nsd_workspace_bytes(most)) || !grow(g.misc, g.misc_cap, 128 + NSD_NCOUNTERS * 8) ||
	    (sll && !grow(g.sll, g.sll_cap, most)) || (ts && !grow(g.ts, g.ts_cap, most)) ||
	    (filter && (!grow(g.desc_out, g.desc_out_cap, most) || !grow(g.verdict, g.verdict_cap, most) ||
			!grow(g.bpf_ws, g.bpf_ws_cap, nsd_bpf_workspace_bytes(most)))))
		return NSD_ERR_NOMEM;
	uint32_t *d_ext_used = (uint32_t *)g.misc, *d_count = (uint32_t *)(g.misc + 64);
	uint64_t *d_counters = (uint64_t *)(g.misc + 128);
	if (!hip_ok(hipMemcpyAsync(g.frames, frames, frames_len, hipMemcpyHostToDevice, s), "H2D") ||
	    !hip_ok(hipMemsetAsync(g.frames + frames_len, 0, NSD_FRAME_PAD, s), "memset"))
		return NSD_ERR_HIP;
	std::vector<uint32_t> verdict;
	std::vector<nsd_sll_t> kept;
	std::vector<uint64_t> kept_ts;
	uint64_t fed = 0;
	for (uint32_t a = 0; a < n; a += CHUNK) {
		const uint32_t m = n - a < CHUNK ? n - a : CHUNK;
		uint32_t m2 = m;
		const uint64_t *use = g.desc;
		const nsd_sll_t *use_sll = sll ? sll + a : nullptr;
		const uint64_t *use_ts = ts ? ts + a : nullptr;
		if (!hip_ok(hipMemcpyAsync(g.desc, desc + a, (size_t)m * 8, hipMemcpyHostToDevice, s), "H2D"))
			return NSD_ERR_HIP;
		if (filter) {
			// bpf_run_filter per record before the dissector (netsniff-ng.c:723-725)
			if (nsd_bpf_filter_device(filter, g.frames, g.desc, m, g.verdict, g.desc_out, d_count, g.bpf_ws, s) !=
			    NSD_OK)
				return NSD_ERR_HIP;
			if (!hip_ok(hipMemcpyAsync(&m2, d_count, 4, hipMemcpyDeviceToHost, s), "D2H") ||
			    !hip_ok(hipStreamSynchronize(s), "sync") || m2 > m)
				return NSD_ERR_HIP;
			use = g.desc_out;
			if ((sll || ts) && m2) {
				// the accepted packets' sockaddr_ll and timestamps, packed like their descriptors
				verdict.resize(m);
				if (!hip_ok(hipMemcpy(verdict.data(), g.verdict, (size_t)m * 4, hipMemcpyDeviceToHost), "D2H"))
					return NSD_ERR_HIP;
				kept.clear();
				kept_ts.clear();
				uint32_t passed = 0;
				for (uint32_t j = 0; j < m; j++) {
					if (!verdict[j])
						continue;
					passed++;
					if (sll)
						kept.push_back(sll[a + j]);
					if (ts)
						kept_ts.push_back(ts[a + j]);
				}
				if (passed != m2)
					return NSD_ERR_HIP;
				if (sll)
					use_sll = kept.data();
				if (ts)
					use_ts = kept_ts.data();
			}
		}
		if (!m2)
			continue;
		if (use_ts && ts_max)
			*ts_max = std::max(*ts_max, *std::max_element(use_ts, use_ts + m2));
		bool ok = hip_ok(hipMemsetAsync(g.misc, 0, 128 + NSD_NCOUNTERS * 8, s), "memset") &&
			  (!use_ts || hip_ok(hipMemcpyAsync(g.ts, use_ts, (size_t)m2 * 8, hipMemcpyHostToDevice, s), "H2D")) &&
			  (!use_sll || hip_ok(hipMemcpyAsync(g.sll, use_sll, (size_t)m2 * sizeof(nsd_sll_t),
							     hipMemcpyHostToDevice, s), "H2D"));
		if (!ok)
			return NSD_ERR_HIP;
		int rc = nsd_dissect_device_sll(g.frames, (const nsd_desc_t *)use, use_sll ? g.sll : nullptr, m2, linktype,
						mode, g.rec, g.ext, ext_words, d_ext_used, d_counters, g.ws, s);
		if (rc == NSD_OK)
			rc = update_device(t, g.frames, (const nsd_desc_t *)use, m2, g.rec, g.ext, ext_words, g.ts, t->timed,
					   base + fed, s);
		if (rc != NSD_OK)
			return rc;
		// (the chunk's buffers are reused by the next one)
		if (!hip_ok(hipStreamSynchronize(s), "sync"))
			return NSD_ERR_HIP;
		fed += m2;
	}
	return (long)fed;
}

extern "C" long nsd_flow_batch(const uint8_t *frames, size_t frames_len, const nsd_desc_t *desc, uint32_t n,
			       int linktype, int mode, nsd_flow *flows, uint32_t max, uint64_t *stats)
{
	if (n > (1u << 30) || (n && (!frames || !desc)) || (max && !flows) || mode < PRINT_NORM || mode > PRINT_NONE)
		return NSD_ERR_ARG;
	nsd_flow_table *t = nsd_flow_create(n ? n : 1);
	if (!t)
		return NSD_ERR_HIP;
	long rc = nsd_flow_feed_host(t, frames, frames_len, desc, nullptr, n, linktype, mode, nullptr, nullptr, nullptr, 0);
	if (rc >= 0)
		rc = nsd_flow_export(t, flows, max, stats);
	nsd_flow_destroy(t);
	return rc;
}
