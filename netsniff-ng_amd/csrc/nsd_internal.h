// nsd_internal.h - everything that crosses a translation unit inside
// libnsdissect.so and is not part of the ABI (include/netsniff_dissect.h).
// Every file that defines or uses one of these includes this header, so a
// declaration that drifts from its definition fails to compile (the
// extern "C" ones would otherwise link and misbehave).  Each symbol's
// visibility is settled here: the launchers stay exported (tools call them),
// NSD_HIDDEN ones are the library's own.
#ifndef NSD_INTERNAL_H
#define NSD_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/netsniff_dissect.h"

#define NSD_HIDDEN __attribute__((visibility("hidden")))

// ---- HIP helpers of the host code ------------------------------------------
NSD_HIDDEN inline bool hip_ok(hipError_t e, const char *what)
{
	if (e != hipSuccess) {
		fprintf(stderr, "netsniff-dissect: %s: %s\n", what, hipGetErrorString(e));
		return false;
	}
	return true;
}

// a device buffer of at least `need` elements (contents not kept); on failure
// p is NULL and cap 0
template <class T>
NSD_HIDDEN inline bool grow(T *&p, size_t &cap, size_t need)
{
	if (need <= cap)
		return true;
	if (p)
		(void)hipFree(p);
	p = nullptr;
	cap = 0;
	const size_t want = need + need / 4 + 64;
	if (!hip_ok(hipMalloc(&p, want * sizeof(T)), "hipMalloc"))
		return false;
	cap = want;
	return true;
}

// the bytes of the frame buffer a batch's descriptors reach
inline size_t batch_extent(const nsd_desc_t *desc, size_t n)
{
	size_t used = 0;
	for (size_t j = 0; j < n; j++) {
		const size_t e = NSD_DESC_OFF(desc[j]) + NSD_DESC_CAPLEN(desc[j]);
		used = e > used ? e : used;
	}
	return used;
}

// ---- the kernels' launcher (nsd_launch.hip) -----------------------------------
// d_sll: one struct sockaddr_ll (nsd_sll_t, 20 bytes) per packet, or NULL
// (read as zeros); d_rec: n nsd_rec (16 B), or n nsd_crec (8 B) when `compact`
extern "C" int nsd_launch_dissect_rec(const uint8_t *d_frames, const uint64_t *d_desc, const void *d_sll,
				      uint32_t n, int start_id, int mode, void *d_rec, int compact, uint32_t *d_ext,
				      uint32_t ext_words, uint32_t *d_ext_used, uint64_t *d_counters, void *d_ws,
				      int grid, hipStream_t stream);
extern "C" size_t nsd_launch_workspace_bytes(uint32_t n);
// the byte offsets and extents of everything a launch of n packets on a grid
// of `blocks` keeps in the workspace (out[20]: see the definition), for tests
extern "C" int nsd_launch_workspace_layout(uint32_t n, uint32_t blocks, int compact, uint64_t *out);
// 1 when the current device's last launch ran the split kernel with a shared tail (tests)
extern "C" int nsd_last_tail_shared(void);

// ---- host paths ------------------------------------------------------------
// linktype -> first ops (nsd_host.cpp)
NSD_HIDDEN int nsd_start_for(int linktype);
// a cached pipe for another file: 0, or 1 when it lives on another device
// than the current one (nsd_pipe.cpp)
extern "C" NSD_HIDDEN int nsd_pipe_retarget(nsd_pipe *p, int linktype, int mode);

// ---- the flow table (nsd_flow.hip) and its host form (nsd_flow_cpu.cpp) ----------
// What both files agree on, host code: the limit of one update, which row
// types carry times (the _ts forms' nsd_flowt / nsd_convt), the rows' orders.
namespace nsdflow {
constexpr uint32_t MAX_N = 0xFFFFFFF0u;   // the most packets of one update

template <class Row>
constexpr bool with_times()
{
	return std::is_same<Row, nsd_flowt>::value || std::is_same<Row, nsd_convt>::value;
}

template <class Row>
static void sort_by_first(std::vector<Row> &v)
{
	std::sort(v.begin(), v.end(), [](const Row &a, const Row &b) { return a.first < b.first; });
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
} // namespace nsdflow

// the flow table's feeds of host batches (nsd_flow.hip).  ts: the packets'
// timestamps, read for a timed table only (where it must be given); *ts_max
// (may be NULL) is raised to the largest timestamp among the packets fed
extern "C" NSD_HIDDEN long nsd_flow_feed_host(nsd_flow_table *t, const uint8_t *frames, size_t frames_len,
					      const nsd_desc_t *desc, const nsd_sll_t *sll, uint32_t n, int linktype,
					      int mode, const nsd_bpf_prog *filter, const uint64_t *ts, uint64_t *ts_max,
					      uint64_t base);
extern "C" NSD_HIDDEN int nsd_flow_feed_records(nsd_flow_table *t, const uint8_t *frames, size_t frames_len,
						const nsd_desc_t *desc, uint32_t n, const nsd_rec *rec,
						const uint32_t *ext, uint32_t ext_words, const uint64_t *ts, uint64_t base);
// nsd_flow_expire / nsd_flow_expire_ts with room for every flow: the removed
// rows, sorted by `first`, into `rows` (nsd_flow.hip, "expiry: the entries";
// the capture-file loop's, nsd_replay.cpp)
NSD_HIDDEN long nsd_flow_expire_rows(nsd_flow_table *t, uint64_t before, uint32_t flags, uint32_t max,
				     std::vector<nsd_flow> &rows, uint64_t *stats);
NSD_HIDDEN long nsd_flow_expire_rows_ts(nsd_flow_table *t, uint64_t before_ns, uint32_t flags, uint32_t max,
					std::vector<nsd_flowt> &rows, uint64_t *stats);

// what dissector_cleanup_all (nsd_proto.cpp) lets go of: the interface name
// cache (nsd_format.cpp; each replay resets it too), the replay's cached
// staging (nsd_replay.cpp), the batch entries' device context (nsd_host.cpp)
extern "C" NSD_HIDDEN void nsd_if_cache_reset(void);
extern "C" NSD_HIDDEN void nsd_replay_release(void);
extern "C" NSD_HIDDEN void nsd_device_ctx_release(void);

// ---- host formatter (nsd_format.cpp) and CPU walk (nsd_cpu.hip) -------------
namespace nsd {
bool render_layer(std::string &s, const uint8_t *pkt, uint32_t caplen, int id, uint32_t start, uint32_t tail,
		  int mode, uint16_t ip_csum, bool icmp_bad, const nsd_sll_t *sll, uint32_t &data,
		  uint32_t &ntail, bool &next);
void render_hex(std::string &s, const uint8_t *pkt, uint32_t caplen, uint32_t from, uint32_t len);
void render_ascii(std::string &s, const uint8_t *pkt, uint32_t caplen, uint32_t from, uint32_t len);
void format_frame_hdr(std::string &s, const nsd_frame_hdr_t &fh, const nsd_sll_t *sll, const uint8_t *pkt,
		      uint32_t caplen, int linktype, int mode, uint64_t count);
int render_packet_cpu(std::string &text, const uint8_t *packet, size_t len, int linktype, int mode,
		      const nsd_sll_t *sll);
int format_replay_part(std::string &s, const uint8_t *frames, const nsd_desc_t *desc, const nsd_frame_hdr_t *fh,
		       const nsd_sll_t *sll, const nsd_crec *rec, const uint32_t *ext, uint64_t count0, uint32_t lo,
		       uint32_t hi, int linktype, int mode);
int cpu_step(int mode, const uint8_t *pkt, uint32_t caplen, int id, uint32_t &data, uint32_t &tail,
	     uint16_t &ip_csum, uint8_t &flags, const nsd_sll_t *sll);
void cpu_count_packet(const uint8_t *pkt, uint32_t caplen, int linktype, int mode, const nsd_sll_t *sll,
		      uint64_t *counters);
} // namespace nsd

#endif
