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
#include <hip/hip_runtime.h>
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
