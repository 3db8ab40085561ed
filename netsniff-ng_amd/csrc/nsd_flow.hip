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
#include <vector>

#include "nsd_flow.h"
#include "nsd_internal.h"

// the device code, one translation unit
#include "nsd_flow_table.h"
#include "nsd_flow_conv.h"
#include "nsd_flow_expire.h"

namespace nsdflow {

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

// How the synchronous entries begin: the table's stats in host memory, after
// everything enqueued on t->last (st[NSD_FLOW_ST_FLOWS] = the flows it holds).
static bool stats_to_host(const nsd_flow_table *t, uint64_t st[NSD_FLOW_NSTATS])
{
	return hip_ok(hipMemcpyAsync(st, t->tab.stats, NSD_FLOW_NSTATS * 8, hipMemcpyDeviceToHost, t->last), "D2H") &&
	       hip_ok(hipStreamSynchronize(t->last), "sync");
}

// The device memory of one synchronous entry, freed when the entry returns:
// 256 bytes for what the device entry counts (and export's stats, at 64), the
// rows, and behind them, 256-aligned, the device entry's workspace.
struct Scratch {
	uint8_t *d = nullptr;
	size_t o_ws = 0;

	Scratch() = default;
	Scratch(const Scratch &) = delete;
	Scratch &operator=(const Scratch &) = delete;
	~Scratch() { (void)hipFree(d); }

	bool alloc(size_t row_bytes, size_t ws_bytes)
	{
		o_ws = (256 + row_bytes + 255) & ~(size_t)255;
		return hip_ok(hipMalloc(&d, o_ws + ws_bytes), "hipMalloc");
	}
	uint32_t *count() const { return (uint32_t *)d; }
	template <class Row>
	Row *rows() const { return (Row *)(d + 256); }
	uint8_t *ws() const { return d + o_ws; }
};

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
static long export_host(nsd_flow_table *t, Row *flows, uint32_t max, uint64_t *stats)
{
	if (!t || (with_times<Row>() && !t->timed) || (max && !flows))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!stats_to_host(t, st))
		return NSD_ERR_HIP;
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS];
	Scratch m;
	if (!m.alloc((size_t)have * sizeof(Row), 0))
		return NSD_ERR_NOMEM;
	uint64_t *d_stats = (uint64_t *)(m.d + 64);
	Row *d_flows = m.rows<Row>();
	std::vector<Row> rows(have);
	uint32_t count = 0;
	const bool ok = export_device(t, d_flows, have, m.count(), d_stats, s, with_times<Row>()) == NSD_OK &&
			hip_ok(hipMemcpyAsync(&count, m.count(), 4, hipMemcpyDeviceToHost, s), "D2H") &&
			hip_ok(hipMemcpyAsync(st, d_stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") &&
			(!have || hip_ok(hipMemcpyAsync(rows.data(), d_flows, (size_t)have * sizeof(Row),
							hipMemcpyDeviceToHost, s), "D2H")) &&
			hip_ok(hipStreamSynchronize(s), "sync");
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

template <class Conv>
static long conversations_host(nsd_flow_table *t, int by, uint32_t k, Conv *conv, uint64_t *stats)
{
	if (!t || (with_times<Conv>() && !t->timed) || by < NSD_CONV_BY_FIRST || by > NSD_CONV_BY_PKTS || (k && !conv))
		return NSD_ERR_ARG;
	hipStream_t s = t->last;
	uint64_t st[NSD_FLOW_NSTATS];
	if (!stats_to_host(t, st))
		return NSD_ERR_HIP;
	// (no more conversations than flows)
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS], want = k < have ? k : have;
	Scratch m;
	if (!m.alloc((size_t)want * sizeof(Conv), nsd_flow_conv_workspace_bytes(t)))
		return NSD_ERR_NOMEM;
	Conv *d_rows = m.rows<Conv>();
	uint32_t count[2] = { 0, 0 };
	std::vector<Conv> rows;
	bool ok = conv_device(t, by, want, d_rows, m.count(), m.ws(), s, with_times<Conv>()) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(count, m.count(), 8, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipStreamSynchronize(s), "sync") && count[0] <= want;
	if (ok && count[0]) {
		rows.resize(count[0]);
		ok = hip_ok(hipMemcpy(rows.data(), d_rows, (size_t)count[0] * sizeof(Conv), hipMemcpyDeviceToHost), "D2H");
	}
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
	if (!stats_to_host(t, st))
		return NSD_ERR_HIP;
	// (no more rows than flows)
	const uint32_t have = (uint32_t)st[NSD_FLOW_ST_FLOWS], want = max < have ? max : have;
	Scratch m;
	if (!m.alloc((size_t)want * sizeof(Row), nsd_flow_expire_workspace_bytes(t)))
		return NSD_ERR_NOMEM;
	Row *d_rows = m.rows<Row>();
	uint32_t count[2] = { 0, 0 };
	ExpHdr h{};
	bool ok = expire_device(t, before, flags, d_rows, want, m.count(), m.ws(), s, with_times<Row>()) == NSD_OK &&
		  hip_ok(hipMemcpyAsync(count, m.count(), 8, hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(&h, m.ws(), sizeof(h), hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipMemcpyAsync(st, t->tab.stats, sizeof(st), hipMemcpyDeviceToHost, s), "D2H") &&
		  hip_ok(hipStreamSynchronize(s), "sync") && count[0] <= want;
	if (ok && count[0]) {
		rows.resize(count[0]);
		ok = hip_ok(hipMemcpy(rows.data(), d_rows, (size_t)count[0] * sizeof(Row), hipMemcpyDeviceToHost), "D2H");
	}
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

// ---- host-memory entries --------------------------------------------------
// Records made on the host (a record no batch carries, walked by the
// per-packet path) into the table: n packets of `frames` with their records
// and ext pool; ts[n] = their timestamps, for a timed table (else ignored).
// Synchronous.
int nsd_flow_feed_records(nsd_flow_table *t, const uint8_t *frames, size_t frames_len, const nsd_desc_t *desc, uint32_t n,
			  const nsd_rec *rec, const uint32_t *ext, uint32_t ext_words, const uint64_t *ts, uint64_t base)
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
long nsd_flow_feed_host(nsd_flow_table *t, const uint8_t *frames, size_t frames_len, const nsd_desc_t *desc,
			const nsd_sll_t *sll, uint32_t n, int linktype, int mode, const nsd_bpf_prog *filter, const uint64_t *ts,
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
