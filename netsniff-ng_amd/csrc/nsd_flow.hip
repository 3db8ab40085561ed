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
//   cnt[slots]  40 B : pkts, bytes, first, last (u64), flags (u32).
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

// what the kernels need of a table
struct Tab {
	uint32_t *state;
	uint64_t *key;
	Cnt *cnt;
	uint64_t *stats;
	uint32_t slots;
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

__global__ __launch_bounds__(BLOCK) void flow_reset(Tab t)
{
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
	for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.slots; s += stride) {
		t.state[s] = EMPTY;
		Cnt c;
		c.pkts = c.bytes = c.last = 0;
		c.first = UINT64_MAX;
		c.flags = c.pad = 0;
		t.cnt[s] = c;
	}
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

__device__ __forceinline__ void add_flow(const Tab &t, const In &in, Agg *agg, uint32_t slot, uint32_t pkts,
					 uint32_t bytes, uint32_t first, uint32_t last, uint32_t flags)
{
	const uint32_t e = slot & (AGG_N - 1);
	const uint32_t old = atomicCAS(&agg->tag[e], NOSLOT, slot);
	if (old == NOSLOT || old == slot) {
		atomicAdd(&agg->pkts[e], pkts);
		atomicAdd(&agg->bytes[e], (unsigned long long)bytes);
		atomicMin(&agg->first[e], first);
		atomicMax(&agg->last[e], last);
		if (flags)
			atomicOr(&agg->flags[e], flags);
		return;
	}
	accumulate(&t.cnt[slot], pkts, bytes, in.base + first, in.base + last, flags);
}

// One packet per lane, grid-stride; the rounds are wave-uniform, so the
// stats are ballots over whole waves.  The block sums in LDS (above) and
// adds its entries to the table after its last packet.
__global__ __launch_bounds__(BLOCK) void flow_update(Tab t, In in)
{
	__shared__ Agg agg_mem;
	Agg *agg = &agg_mem;
	for (uint32_t e = threadIdx.x; e < AGG_N; e += BLOCK) {
		agg->tag[e] = NOSLOT;
		agg->pkts[e] = agg->last[e] = agg->flags[e] = 0;
		agg->first[e] = 0xFFFFFFFFu;
		agg->bytes[e] = 0;
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
		if (found)
			add_flow(t, in, agg, slot, 1, caplen, (uint32_t)i, (uint32_t)i, tflags);
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
		if (slot < t.slots)
			accumulate(&t.cnt[slot], agg->pkts[e], agg->bytes[e], in.base + agg->first[e], in.base + agg->last[e],
				   agg->flags[e]);
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
// zeroed before the launch); rows past `max` are counted, not written.
__global__ __launch_bounds__(BLOCK) void flow_export(Tab t, uint64_t *out, uint32_t max, uint32_t *count,
						     uint64_t *stats_out)
{
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
			uint64_t *o = out + 9ull * pos;
			o[0] = kp[0];
			o[1] = kp[1];
			o[2] = kp[2];
			o[3] = kp[3];
			o[4] = kp[4] | (uint64_t)(c.flags & 0xFFu) << 48;
			o[5] = c.pkts;
			o[6] = c.bytes;
			o[7] = c.first;
			o[8] = c.last;
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
// and k - rem .. k - 1, each through a wave-aggregated cursor.
__global__ __launch_bounds__(BLOCK) void conv_gather(Tab t, ConvWs w, uint32_t k, uint64_t *out, uint32_t *count)
{
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
		uint64_t *o = out + 11ull * pos;
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
// the five key words, then the Cnt.  The kernels bound the counts they read
// from the header by `slots`.
constexpr size_t EXP_HDR = 2048;

struct ExpHdr {
	uint32_t qualified;   // expire_split's cursor of qualifying flows
	uint32_t survivors;   // ... and of the flows that stay
	uint32_t lost;        // survivors that found no slot (cannot happen; the host entry checks)
	uint32_t pad;
};
static_assert(sizeof(ExpHdr) <= EXP_HDR, "expire header");

struct ExpWs {
	ExpHdr *h;
	uint64_t *rows;   // 10 words per survivor
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
__global__ __launch_bounds__(BLOCK) void expire_split(Tab t, ExpWs w, uint64_t before, uint32_t flags, uint64_t *out,
						      uint32_t max)
{
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
		if (occ) {
			load_key(t, (uint32_t)s, k);
			c = t.cnt[s];
			idle = c.last < before;
			if (idle && (flags & NSD_FLOW_EXPIRE_PAIRED)) {
				Key r;
				reverse_key(k, r);
				if (!key_eq(k, r)) {
					const uint32_t rev = find_key(t, r);
					if (rev != NOSLOT)
						idle = t.cnt[rev].last < before;
				}
			}
		}
		const uint64_t mq = __ballot(idle);
		bool stay = occ && !idle;
		if (mq) {
			const uint64_t pos = wave_cursor(&w.h->qualified, mq, lane);
			if (idle) {
				if (pos < max) {
					uint64_t *o = out + 9ull * pos;
					o[0] = k.w[0];
					o[1] = k.w[1];
					o[2] = k.w[2];
					o[3] = k.w[3];
					o[4] = k.w[4] | (uint64_t)(c.flags & 0xFFu) << 48;
					o[5] = c.pkts;
					o[6] = c.bytes;
					o[7] = c.first;
					o[8] = c.last;
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
			uint64_t *o = w.rows + 10ull * pos;
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
	for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < t.slots; s += stride) {
		t.state[s] = EMPTY;
		Cnt c;
		c.pkts = c.bytes = c.last = 0;
		c.first = UINT64_MAX;
		c.flags = c.pad = 0;
		t.cnt[s] = c;
	}
}

// One survivor per lane, grid-stride.  Keys are unique, so a lane never
// compares against a slot: it takes the first EMPTY one of its probe (one
// relaxed CAS; a slot another lane took is passed by) and stores its own rows
// there with plain stores, which nobody reads before the next kernel.
__global__ __launch_bounds__(BLOCK) void expire_reinsert(Tab t, ExpWs w, uint32_t max)
{
	if (!expire_removed(w, max))
		return;
	const uint32_t n = expire_survivors(w);
	const uint32_t mask = t.slots - 1;
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
#pragma unroll 1
	for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
		const uint64_t *r = w.rows + 10ull * i;
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

	void release()
	{
		(void)hipFree(frames); (void)hipFree(desc); (void)hipFree(desc_out); (void)hipFree(verdict);
		(void)hipFree(rec); (void)hipFree(ext); (void)hipFree(ws); (void)hipFree(bpf_ws); (void)hipFree(sll);
		(void)hipFree(misc);
		*this = Stage();
	}
};

} // namespace nsdflow

using namespace nsdflow;

struct nsd_flow_table {
	Tab tab{};
	void *mem = nullptr;
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

extern "C" nsd_flow_table *nsd_flow_create(uint32_t max_flows)
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
	// one allocation: state | stats | key | cnt
	const size_t a = 256;
	auto up = [&](size_t v) { return (v + a - 1) & ~(a - 1); };
	const size_t o_state = 0, o_misc = up((size_t)slots * 4), o_key = o_misc + a, o_cnt = o_key + up((size_t)slots * 40), total = o_cnt + up((size_t)slots * 40);
	if (!hip_ok(hipMalloc(&t->mem, total), "hipMalloc")) {
		delete t;
		return nullptr;
	}
	uint8_t *m = (uint8_t *)t->mem;
	t->tab.state = (uint32_t *)(m + o_state);
	t->tab.stats = (uint64_t *)(m + o_misc);
	t->tab.key = (uint64_t *)(m + o_key);
	t->tab.cnt = (Cnt *)(m + o_cnt);
	t->tab.slots = slots;
	if (nsd_flow_reset(t, nullptr) != NSD_OK || !hip_ok(hipStreamSynchronize(nullptr), "sync")) {
		(void)hipFree(t->mem);
		delete t;
		return nullptr;
	}
	return t;
}

extern "C" void nsd_flow_destroy(nsd_flow_table *t)
{
	if (!t)
		return;
	(void)hipDeviceSynchronize();
	t->stage.release();
	(void)hipFree(t->mem);
	delete t;
}

extern "C" int nsd_flow_update_device(nsd_flow_table *t, const uint8_t *d_frames, const nsd_desc_t *d_desc,
				      uint32_t n, const nsd_rec *d_rec, const uint32_t *d_ext, uint32_t ext_words,
				      uint64_t base, void *stream)
{
	if (!t || n > MAX_N)
		return NSD_ERR_ARG;
	if (n == 0)
		return NSD_OK;
	if (!d_frames || !d_desc || !d_rec || (ext_words && !d_ext))
		return NSD_ERR_ARG;
	if (((uintptr_t)d_rec & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ext & 3))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const In in{ d_frames, (const uint64_t *)d_desc, d_rec, ext_words ? d_ext : nullptr, ext_words, n, base };
	const dim3 grid(grid_for(t, n)), block(BLOCK);
	hipLaunchKernelGGL(flow_update, grid, block, 0, s, t->tab, in);
	hipLaunchKernelGGL(flow_commit, dim3(grid_for(t, t->tab.slots)), block, 0, s, t->tab, in);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

extern "C" int nsd_flow_export_device(nsd_flow_table *t, nsd_flow *d_flows, uint32_t max, uint32_t *d_count,
				      uint64_t *d_stats, void *stream)
{
	if (!t || !d_count || !d_stats || (max && !d_flows) || ((uintptr_t)d_flows & 7))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	if (!hip_ok(hipMemsetAsync(d_count, 0, 4, s), "memset"))
		return NSD_ERR_HIP;
	hipLaunchKernelGGL(flow_export, dim3(grid_for(t, t->tab.slots)), dim3(BLOCK), 0, s, t->tab, (uint64_t *)d_flows,
			   max, d_count, d_stats);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

static void sort_by_first(std::vector<nsd_flow> &v)
{
	std::sort(v.begin(), v.end(), [](const nsd_flow &a, const nsd_flow &b) { return a.first < b.first; });
}

extern "C" long nsd_flow_export(nsd_flow_table *t, nsd_flow *flows, uint32_t max, uint64_t *stats)
{
	if (!t || (max && !flows))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") ||
	    !hip_ok(hipStreamSynchronize(s), "sync"))
		return NSD_ERR_HIP;
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS];
	uint8_t *d = nullptr;
	if (!hip_ok(hipMalloc(&d, 256 + (size_t)have * sizeof(nsd_flow)), "hipMalloc"))
		return NSD_ERR_NOMEM;
	uint32_t *d_count = (uint32_t *)d;
	uint64_t *d_stats = (uint64_t *)(d + 64);
	nsd_flow *d_flows = (nsd_flow *)(d + 256);
	std::vector<nsd_flow> rows(have);
	uint32_t count = 0;
	bool ok = nsd_flow_export_device(t, d_flows, have, d_count, d_stats, s) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") &&
		  (!have || hip_ok(hipMemcpyAsync(rows.data(), d_flows, (size_t)have * sizeof(nsd_flow),
						  hipMemcpyDeviceToHost, s), "D2H")) &&
		  hip_ok(hipStreamSynchronize(s), "sync");
	(void)hipFree(d);
	if (!ok || count != have)
		return NSD_ERR_HIP;
	sort_by_first(rows);
	const uint32_t k = have < max ? have : max;
	if (k)
		memcpy(flows, rows.data(), (size_t)k * sizeof(nsd_flow));
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)have;
}

// ---- conversations: the entries ---------------------------------------------
static_assert(sizeof(nsd_conv) == 88 && offsetof(nsd_conv, pkts_src) == 40, "nsd_conv");

extern "C" size_t nsd_flow_conv_workspace_bytes(const nsd_flow_table *t)
{
	return t ? CONV_HDR + 24 * (size_t)t->tab.slots : 0;
}

// init | pair | per digit: hist, scan | gather: a linear chain of kernels on `stream`
extern "C" int nsd_flow_conv_device(nsd_flow_table *t, int by, uint32_t k, nsd_conv *d_conv, uint32_t *d_count,
				    void *d_workspace, void *stream)
{
	if (!t || by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || !d_count || !d_workspace ||
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
	hipLaunchKernelGGL(conv_gather, grid, block, 0, s, t->tab, w, k, (uint64_t *)d_conv, d_count);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

// the total order of the header: `by`'s metric descending, then first ascending
static void sort_conv(std::vector<nsd_conv> &v, int by)
{
	std::sort(v.begin(), v.end(), [by](const nsd_conv &a, const nsd_conv &b) {
		if (by != NSD_CONV_BY_FIRST) {
			const uint64_t ma = by == NSD_CONV_BY_BYTES ? a.bytes_src + a.bytes_dst : a.pkts_src + a.pkts_dst;
			const uint64_t mb = by == NSD_CONV_BY_BYTES ? b.bytes_src + b.bytes_dst : b.pkts_src + b.pkts_dst;
			if (ma != mb)
				return ma > mb;
		}
		return a.first < b.first;
	});
}

extern "C" long nsd_flow_conversations(nsd_flow_table *t, int by, uint32_t k, nsd_conv *conv, uint64_t *stats)
{
	if (!t || by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || (k && !conv))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") ||
	    !hip_ok(hipStreamSynchronize(s), "sync"))
		return NSD_ERR_HIP;
	// (no more conversations than flows)
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS], want = k < have ? k : have;
	const size_t o_rows = 256, o_ws = (o_rows + (size_t)want * sizeof(nsd_conv) + 255) & ~(size_t)255;
	uint8_t *d = nullptr;
	if (!hip_ok(hipMalloc(&d, o_ws + nsd_flow_conv_workspace_bytes(t)), "hipMalloc"))
		return NSD_ERR_NOMEM;
	uint32_t *d_count = (uint32_t *)d;
	nsd_conv *d_rows = (nsd_conv *)(d + o_rows);
	uint32_t count[2] = { 0, 0 };
	std::vector<nsd_conv> rows;
	bool ok = nsd_flow_conv_device(t, by, want, d_rows, d_count, d + o_ws, s) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(count, d_count, 8, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipStreamSynchronize(s), "sync") && count[0] <= want;
	if (ok && count[0]) {
		rows.resize(count[0]);
		ok = hip_ok(hipMemcpy(rows.data(), d_rows, (size_t)count[0] * sizeof(nsd_conv), hipMemcpyDeviceToHost), "D2H");
	}
	(void)hipFree(d);
	if (!ok)
		return NSD_ERR_HIP;
	sort_conv(rows, by);
	if (!rows.empty())
		memcpy(conv, rows.data(), rows.size() * sizeof(nsd_conv));
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)count[1];
}

// ---- expiry: the entries ------------------------------------------------------
extern "C" size_t nsd_flow_expire_workspace_bytes(const nsd_flow_table *t)
{
	return t ? EXP_HDR + 80 * (size_t)t->tab.slots : 0;
}

// init | split | clear | reinsert: a linear chain of kernels on `stream`
extern "C" int nsd_flow_expire_device(nsd_flow_table *t, uint64_t before, uint32_t flags, nsd_flow *d_expired,
				      uint32_t max, uint32_t *d_count, void *d_workspace, void *stream)
{
	if (!t || (flags & ~NSD_FLOW_EXPIRE_PAIRED) || !d_count || !d_workspace || (max && !d_expired) ||
	    ((uintptr_t)d_expired & 7) || ((uintptr_t)d_workspace & 15) || ((uintptr_t)d_count & 3))
		return NSD_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	uint8_t *m = (uint8_t *)d_workspace;
	const ExpWs w{ (ExpHdr *)m, (uint64_t *)(m + EXP_HDR), t->tab.slots };
	const dim3 grid(grid_for(t, t->tab.slots)), block(BLOCK);
	hipLaunchKernelGGL(expire_init, dim3(1), block, 0, s, w);
	hipLaunchKernelGGL(expire_split, grid, block, 0, s, t->tab, w, before, flags, (uint64_t *)d_expired, max);
	hipLaunchKernelGGL(expire_clear, grid, block, 0, s, t->tab, w, max, d_count);
	hipLaunchKernelGGL(expire_reinsert, grid, block, 0, s, t->tab, w, max);
	t->last = s;
	return hip_ok(hipGetLastError(), "launch") ? NSD_OK : NSD_ERR_HIP;
}

long nsd_flow_expire_rows(nsd_flow_table *t, uint64_t before, uint32_t flags, uint32_t max,
			  std::vector<nsd_flow> &rows, uint64_t *stats)
{
	rows.clear();
	if (!t || (flags & ~NSD_FLOW_EXPIRE_PAIRED))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") ||
	    !hip_ok(hipStreamSynchronize(s), "sync"))
		return NSD_ERR_HIP;
	// (no more rows than flows)
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS], want = max < have ? max : have;
	const size_t o_rows = 256, o_ws = (o_rows + (size_t)want * sizeof(nsd_flow) + 255) & ~(size_t)255;
	uint8_t *d = nullptr;
	if (!hip_ok(hipMalloc(&d, o_ws + nsd_flow_expire_workspace_bytes(t)), "hipMalloc"))
		return NSD_ERR_NOMEM;
	uint32_t *d_count = (uint32_t *)d;
	nsd_flow *d_rows = (nsd_flow *)(d + o_rows);
	uint32_t count[2] = { 0, 0 };
	ExpHdr h{};
	bool ok = nsd_flow_expire_device(t, before, flags, d_rows, want, d_count, d + o_ws, s) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(count, d_count, 8, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(&h, d + o_ws, sizeof(h), hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipStreamSynchronize(s), "sync") && count[0] <= want;
	if (ok && count[0]) {
		rows.resize(count[0]);
		ok = hip_ok(hipMemcpy(rows.data(), d_rows, (size_t)count[0] * sizeof(nsd_flow), hipMemcpyDeviceToHost), "D2H");
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

extern "C" long nsd_flow_expire(nsd_flow_table *t, uint64_t before, uint32_t flags, nsd_flow *expired, uint32_t max,
				uint64_t *stats)
{
	if (max && !expired)
		return NSD_ERR_ARG;
	std::vector<nsd_flow> rows;
	const long q = nsd_flow_expire_rows(t, before, flags, max, rows, stats);
	if (q >= 0 && !rows.empty())
		memcpy(expired, rows.data(), rows.size() * sizeof(nsd_flow));
	return q;
}

// ---- the same aggregation on the host -----------------------------------
namespace {
struct KeyHash {
	size_t operator()(const Key &k) const { return (size_t)key_hash(k); }
};
struct KeyEq {
	bool operator()(const Key &a, const Key &b) const { return key_eq(a, b); }
};
} // namespace

extern "C" long nsd_flow_cpu(const uint8_t *frames, const nsd_desc_t *desc, uint32_t n, const nsd_rec *rec,
			     const uint32_t *ext, uint64_t base, nsd_flow *flows, uint32_t max, uint64_t *stats)
{
	if (n > MAX_N || (n && (!frames || !desc || !rec)) || (max && !flows))
		return NSD_ERR_ARG;
	std::unordered_map<Key, nsd_flow, KeyHash, KeyEq> map;
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
			nsd_flow f;
			memset(&f, 0, sizeof(f));
			memcpy(&f, k.w, 40);
			f.first = base + i;
			it = map.emplace(k, f).first;
		}
		nsd_flow &f = it->second;
		f.pkts++;
		f.bytes += caplen;
		f.last = base + i;
		f.tcp_flags |= (uint8_t)tf;
	}
	st[NSD_FLOW_ST_FLOWS] = map.size();
	std::vector<nsd_flow> rows;
	rows.reserve(map.size());
	for (const auto &kv : map)
		rows.push_back(kv.second);
	sort_by_first(rows);
	const size_t k = rows.size() < max ? rows.size() : max;
	if (k)
		memcpy(flows, rows.data(), k * sizeof(nsd_flow));
	if (stats)
		memcpy(stats, st, sizeof(st));
	return (long)rows.size();
}

// Flow rows (unique keys, any order) paired into conversations on the host:
// a hash map from key to row, one lookup of the reverse per row.
extern "C" long nsd_conv_cpu(const nsd_flow *flows, size_t n, int by, nsd_conv *conv, uint32_t max)
{
	if (by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || (n && !flows) || (max && !conv))
		return NSD_ERR_ARG;
	auto key_of = [](const nsd_flow &f) {
		Key k;
		memcpy(k.w, &f, 40);
		k.w[4] &= 0x0000FFFFFFFFFFFFull;   // tcp_flags, rsvd
		return k;
	};
	std::unordered_map<Key, size_t, KeyHash, KeyEq> map;
	map.reserve(n);
	for (size_t i = 0; i < n; i++)
		map.emplace(key_of(flows[i]), i);
	std::vector<nsd_conv> rows;
	for (size_t i = 0; i < n; i++) {
		const nsd_flow &f = flows[i];
		nsd_flow r = f;
		memcpy(r.src, f.dst, 16);
		memcpy(r.dst, f.src, 16);
		r.sport = f.dport;
		r.dport = f.sport;
		const Key k = key_of(f), kr = key_of(r);
		const auto it = key_eq(k, kr) ? map.end() : map.find(kr);
		const nsd_flow *g = it == map.end() ? nullptr : &flows[it->second];
		if (g && (g->first < f.first || (g->first == f.first && memcmp(kr.w, k.w, 40) < 0)))
			continue;   // the reverse is the originator: its row carries this one
		nsd_conv c;
		memset(&c, 0, sizeof(c));
		memcpy(&c, k.w, 40);
		c.tcp_flags_src = f.tcp_flags;
		c.pkts_src = f.pkts;
		c.bytes_src = f.bytes;
		c.first = f.first;
		c.last = f.last;
		if (g) {
			c.tcp_flags_dst = g->tcp_flags;
			c.pkts_dst = g->pkts;
			c.bytes_dst = g->bytes;
			c.last = g->last > f.last ? g->last : f.last;
		}
		rows.push_back(c);
	}
	sort_conv(rows, by);
	const size_t k = rows.size() < max ? rows.size() : max;
	if (k)
		memcpy(conv, rows.data(), k * sizeof(nsd_conv));
	return (long)rows.size();
}

// The expiry rules on the host over flow rows (unique keys, any order): a hash
// map from key to row for the reverse lookup.  Survivors keep their input
// order at the front of `flows`; the first `max` qualifying rows in input
// order go to `expired`, the others stay.
extern "C" long nsd_flow_expire_cpu(nsd_flow *flows, size_t n, uint64_t before, uint32_t flags, nsd_flow *expired,
				    uint32_t max, size_t *remaining)
{
	if ((flags & ~NSD_FLOW_EXPIRE_PAIRED) || (n && !flows) || (max && !expired) || !remaining)
		return NSD_ERR_ARG;
	auto key_of = [](const nsd_flow &f) {
		Key k;
		memcpy(k.w, &f, 40);
		k.w[4] &= 0x0000FFFFFFFFFFFFull;   // tcp_flags, rsvd
		return k;
	};
	std::unordered_map<Key, size_t, KeyHash, KeyEq> map;
	if (flags & NSD_FLOW_EXPIRE_PAIRED) {
		map.reserve(n);
		for (size_t i = 0; i < n; i++)
			map.emplace(key_of(flows[i]), i);
	}
	// decided over the rows as given, before any of them moves
	std::vector<uint8_t> idle(n);
	for (size_t i = 0; i < n; i++) {
		const nsd_flow &f = flows[i];
		idle[i] = f.last < before;
		if (!idle[i] || !(flags & NSD_FLOW_EXPIRE_PAIRED))
			continue;
		nsd_flow r = f;
		memcpy(r.src, f.dst, 16);
		memcpy(r.dst, f.src, 16);
		r.sport = f.dport;
		r.dport = f.sport;
		const Key k = key_of(f), kr = key_of(r);
		const auto it = key_eq(k, kr) ? map.end() : map.find(kr);
		if (it != map.end())
			idle[i] = flows[it->second].last < before;
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

// ---- host-memory entries --------------------------------------------------
// Records made on the host (a record no batch carries, walked by the
// per-packet path) into the table: n packets of `frames` with their records
// and ext pool.  Synchronous.
extern "C" __attribute__((visibility("hidden"))) int nsd_flow_feed_records(nsd_flow_table *t, const uint8_t *frames,
									    size_t frames_len, const nsd_desc_t *desc,
									    uint32_t n, const nsd_rec *rec,
									    const uint32_t *ext, uint32_t ext_words,
									    uint64_t base)
{
	if (!t || !n)
		return t ? NSD_OK : NSD_ERR_ARG;
	Stage &g = t->stage;
	hipStream_t s = t->last;
	if (!grow(g.frames, g.frames_cap, frames_len + NSD_FRAME_PAD) || !grow(g.desc, g.desc_cap, n) ||
	    !grow(g.rec, g.rec_cap, n) || (ext_words && !grow(g.ext, g.ext_cap, ext_words)))
		return NSD_ERR_NOMEM;
	bool ok = hip_ok(hipMemcpyAsync(g.frames, frames, frames_len, hipMemcpyHostToDevice, s), "H2D") &&
		  hip_ok(hipMemsetAsync(g.frames + frames_len, 0, NSD_FRAME_PAD, s), "memset") &&
		  hip_ok(hipMemcpyAsync(g.desc, desc, (size_t)n * 8, hipMemcpyHostToDevice, s), "H2D") &&
		  hip_ok(hipMemcpyAsync(g.rec, rec, (size_t)n * sizeof(nsd_rec), hipMemcpyHostToDevice, s), "H2D") &&
		  (!ext_words || hip_ok(hipMemcpyAsync(g.ext, ext, (size_t)ext_words * 4, hipMemcpyHostToDevice, s), "H2D"));
	if (!ok)
		return NSD_ERR_HIP;
	const int rc = nsd_flow_update_device(t, g.frames, g.desc, n, g.rec, g.ext, ext_words, base, s);
	if (rc != NSD_OK)
		return rc;
	return hip_ok(hipStreamSynchronize(s), "sync") ? NSD_OK : NSD_ERR_HIP;
}

// A host-memory batch into the table: staged, filtered by the optional BPF
// program (accepted descriptors packed on the device, nsd_bpf_filter_device),
// walked and accumulated, in chunks whose ext pool stays small.  The packets
// fed get base, base + 1, ...  Returns their number or a negative NSD_ERR_*.
// Synchronous.
extern "C" __attribute__((visibility("hidden"))) long nsd_flow_feed_host(nsd_flow_table *t, const uint8_t *frames,
									  size_t frames_len, const nsd_desc_t *desc,
									  const nsd_sll_t *sll, uint32_t n, int linktype,
									  int mode, const nsd_bpf_prog *filter, uint64_t base)
{
	if (!t || mode < PRINT_NORM || mode > PRINT_NONE || (n && (!frames || !desc)))
		return NSD_ERR_ARG;
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
	    (sll && !grow(g.sll, g.sll_cap, most)) ||
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
	uint64_t fed = 0;
	for (uint32_t a = 0; a < n; a += CHUNK) {
		const uint32_t m = n - a < CHUNK ? n - a : CHUNK;
		uint32_t m2 = m;
		const uint64_t *use = g.desc;
		const nsd_sll_t *use_sll = sll ? sll + a : nullptr;
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
			if (sll && m2) {
				// the accepted packets' sockaddr_ll, packed like their descriptors
				verdict.resize(m);
				if (!hip_ok(hipMemcpy(verdict.data(), g.verdict, (size_t)m * 4, hipMemcpyDeviceToHost), "D2H"))
					return NSD_ERR_HIP;
				kept.clear();
				for (uint32_t j = 0; j < m; j++)
					if (verdict[j])
						kept.push_back(sll[a + j]);
				if (kept.size() != m2)
					return NSD_ERR_HIP;
				use_sll = kept.data();
			}
		}
		if (!m2)
			continue;
		bool ok = hip_ok(hipMemsetAsync(g.misc, 0, 128 + NSD_NCOUNTERS * 8, s), "memset") &&
			  (!use_sll || hip_ok(hipMemcpyAsync(g.sll, use_sll, (size_t)m2 * sizeof(nsd_sll_t),
							     hipMemcpyHostToDevice, s), "H2D"));
		if (!ok)
			return NSD_ERR_HIP;
		int rc = nsd_dissect_device_sll(g.frames, (const nsd_desc_t *)use, use_sll ? g.sll : nullptr, m2, linktype,
						mode, g.rec, g.ext, ext_words, d_ext_used, d_counters, g.ws, s);
		if (rc == NSD_OK)
			rc = nsd_flow_update_device(t, g.frames, (const nsd_desc_t *)use, m2, g.rec, g.ext, ext_words,
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
	long rc = nsd_flow_feed_host(t, frames, frames_len, desc, nullptr, n, linktype, mode, nullptr, 0);
	if (rc >= 0)
		rc = nsd_flow_export(t, flows, max, stats);
	nsd_flow_destroy(t);
	return rc;
}
