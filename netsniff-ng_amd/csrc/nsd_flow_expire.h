// nsd_flow_expire.h - flow expiry: device code of nsd_flow.hip's translation
// unit, after nsd_flow_table.h.
//
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
#ifndef NSD_FLOW_EXPIRE_H
#define NSD_FLOW_EXPIRE_H

#include "nsd_flow_table.h"

namespace nsdflow {

constexpr size_t EXP_HDR = 2048;
constexpr uint64_t exp_row_words(bool tt) { return tt ? 12 : 10; }

// a survivor's row: key | pkts, bytes, first, last, flags | TT: t_first, t_last
template <bool TT>
__device__ __forceinline__ void pack_survivor(uint64_t *o, const Key &k, const Cnt &c, uint64_t t_first, uint64_t t_last)
{
	for (int j = 0; j < 5; j++)
		o[j] = k.w[j];
	o[5] = c.pkts;
	o[6] = c.bytes;
	o[7] = c.first;
	o[8] = c.last;
	o[9] = c.flags;
	if constexpr (TT) {
		o[10] = t_first;
		o[11] = t_last;
	}
}
// ... and back, in two parts: expire_reinsert probes with the key and reads
// the rest only when it has a slot to put it in (read earlier, the words wait
// in registers through the probe)
__device__ __forceinline__ void unpack_survivor_key(const uint64_t *r, Key &k)
{
	for (int j = 0; j < 5; j++)
		k.w[j] = r[j];
}
template <bool TT>
__device__ __forceinline__ void unpack_survivor_into(const uint64_t *r, const Tab &t, uint32_t slot)
{
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
					store_flow_row(o, k, c);
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
		if (stay && max && pos < t.slots)
			pack_survivor<TT>(w.rows + KEEP * pos, k, c, tf, tl);
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
		unpack_survivor_key(r, k);
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
		store_key(t, slot, k);
		unpack_survivor_into<TT>(r, t, slot);
	}
}

} // namespace nsdflow

#endif /* NSD_FLOW_EXPIRE_H */
