// nsd_replay.cpp - what drives the pcap reader (nsd_pcap.cpp): the replay
// (`netsniff-ng --in file.pcap [--out f.pcap]`, read_pcap
// netsniff-ng.c:640-770), which feeds the reader's batches through the
// optional device BPF filter and the pipelined device walk (nsd_pipe_*) and
// writes the formatted text, and the flow table's loop over a file
// (nsd_pcap_flows).
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <sys/uio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "nsd_pcap_reader.h"

using namespace nsd::reader;

namespace {

bool write_all(int fd, const void *buf, size_t n)
{
	const uint8_t *w = (const uint8_t *)buf;
	while (n) {
		ssize_t r = write(fd, w, n);
		if (r < 0 && errno == EINTR)
			continue;
		if (r <= 0)
			return false;
		w += r;
		n -= (size_t)r;
	}
	return true;
}

// pcap_generic_push_fhdr -> pcap_prepare_header (pcap_io.h:813-843, 936-950)
// with the replayed file's magic and link type as read_pcap holds them
// (ctx->magic / ctx->link_type, netsniff-ng.c:694-695): the *_LL remap undone
// (the stored magic), version 2.4, thiszone 0, sigfigs 0, snaplen 65535,
// link type swapped once more when the magic is a swapped one (as the
// reference does with the as-stored value).  A swapped SLL / netlink file
// holds the remapped magic swab32(*_MAGIC_LL), which pcap_magic_is_swapped
// does not recognise (pcap_io.h:307-320): its header is written unswapped,
// the link type as stored.
bool push_fhdr(const nsd_pcap *p, int fd)
{
	uint8_t h[24];
	const bool sw = p->swapped && p->ll_extra == 0;
	const uint16_t vmaj = sw ? __builtin_bswap16(2) : 2, vmin = sw ? __builtin_bswap16(4) : 4;
	const uint32_t zero = 0, snap = sw ? __builtin_bswap32(65535) : 65535;
	const uint32_t lt = sw ? __builtin_bswap32(p->linktype) : p->linktype;
	memcpy(h, &p->magic_raw, 4);
	memcpy(h + 4, &vmaj, 2);
	memcpy(h + 6, &vmin, 2);
	memcpy(h + 8, &zero, 4);
	memcpy(h + 12, &zero, 4);
	memcpy(h + 16, &snap, 4);
	memcpy(h + 20, &lt, 4);
	return write_all(fd, h, sizeof(h));
}

// The record after a batch that could not carry it (read_batch / scan_batch
// gave NSD_ERR_CAPLEN): read whole (read_one), then the filter's verdict on
// it alone (bpf_run_filter per record, netsniff-ng.c:723-725; *pass = true
// without a filter).  Returns its caplen, 0 at the end of the replay, or a
// negative NSD_ERR_*.
long read_big(nsd_pcap *p, const nsd_bpf_prog *filter, std::vector<uint8_t> &frame, nsd_sll_t *sll,
	      nsd_frame_hdr_t *fh, uint8_t *rhdr, bool *pass)
{
	*pass = true;
	const long caplen = read_one(p, frame, sll, fh, rhdr);
	if (caplen <= 0 || !filter)
		return caplen;
	const nsd_desc_t d = NSD_DESC(0, caplen);
	uint32_t v = 0;
	const int r = nsd_bpf_filter_batch(filter, frame.data(), (size_t)caplen, &d, 1, &v);
	*pass = v != 0;
	return r != NSD_OK ? r : caplen;
}

} // namespace

// ---- flows of a capture file (the table's feeds and entries: nsd_flow.hip) -------
// read_pcap's loop (netsniff-ng.c:707-756: next record, bpf_run_filter, then
// the dissector) with the flow table where the dissector's text would be:
// batches of the reader go through the device filter / walk / update; a
// record no batch carries is filtered and walked by the per-packet path over
// its first NSD_MAX_CAPLEN bytes and added with its whole caplen.
// Batches carry at most `every` records; after each one fed (a record no
// batch carries is a batch of its own) `after(fed, now)` runs, and a negative
// return of it ends the loop with that status.  A timed table is fed the
// records' timestamps (the reader's ts_ns), and now = the largest one among
// the packets fed so far (0 for a plain table).
namespace {
constexpr uint32_t FLOWS_MAX_N = 1u << 16;

// read_batch's ts_ns of one record header as stored (the record read_one gave)
uint64_t record_ts_ns(const nsd_pcap *p, const uint8_t *rhdr)
{
	uint32_t sec, frac;
	memcpy(&sec, rhdr, 4);
	memcpy(&frac, rhdr + 4, 4);
	if (p->swapped) {
		sec = __builtin_bswap32(sec);
		frac = __builtin_bswap32(frac);
	}
	return (uint64_t)sec * 1000000000ull + (p->nsec ? frac : (uint64_t)frac * 1000ull);
}

template <class After>
long pcap_flows_loop(const char *path, int mode, const nsd_bpf_prog *filter, nsd_flow_table *t, uint32_t every,
		     After after)
{
	if (!path || !t || mode < PRINT_NORM || mode > PRINT_NONE || every == 0 || every > FLOWS_MAX_N)
		return NSD_ERR_ARG;
	nsd_pcap *p = nsd_pcap_open(path);
	if (!p)
		return NSD_ERR_ARG;
	const int lt = (int)p->linktype;
	const bool ll_used = has_ll(p), timed = nsd_flow_is_timed(t) != 0;
	constexpr size_t CAP = 16u << 20;
	std::vector<uint8_t> frames(CAP), big;
	std::vector<nsd_desc_t> desc(every);
	std::vector<nsd_sll_t> sll(every);
	std::vector<uint64_t> ts(timed ? every : 0);
	uint64_t fed = 0, now = 0;
	long rc = NSD_OK;
	while (rc == NSD_OK) {
		const long n = read_batch(p, frames.data(), CAP, desc.data(), sll.data(), nullptr, every, nullptr,
					  timed ? ts.data() : nullptr, nullptr);
		if (n == 0)
			break;
		if (n > 0) {
			const long k = nsd_flow_feed_host(t, frames.data(), batch_extent(desc.data(), (size_t)n), desc.data(),
							  ll_used ? sll.data() : nullptr, (uint32_t)n, lt, mode, filter,
							  timed ? ts.data() : nullptr, &now, fed);
			if (k < 0)
				rc = k;
			else
				fed += (uint64_t)k;
			if (rc == NSD_OK)
				rc = after(fed, now);
			continue;
		}
		if (n != NSD_ERR_CAPLEN) {
			rc = n;
			break;
		}
		nsd_sll_t ll;
		bool pass;
		uint8_t rhdr[32];
		const long caplen = read_big(p, filter, big, &ll, nullptr, rhdr, &pass);
		if (caplen <= 0) {
			rc = caplen < 0 ? caplen : NSD_OK;
			break;
		}
		if (!pass)
			continue;
		const nsd_desc_t d = NSD_DESC(0, caplen);
		const uint32_t head = (uint32_t)caplen < NSD_MAX_CAPLEN ? (uint32_t)caplen : NSD_MAX_CAPLEN;
		nsd_rec rec;
		uint32_t ext[NSD_EXT_WORDS(NSD_EXT_MAX_LAYERS)] = { 0 };
		rc = nsd_walk_packet_cpu(big.data(), head, lt, mode, ll_used ? &ll : nullptr, &rec, ext,
					 NSD_EXT_WORDS(NSD_EXT_MAX_LAYERS), nullptr);
		const uint64_t big_ts = record_ts_ns(p, rhdr);
		if (rc == NSD_OK)
			rc = nsd_flow_feed_records(t, big.data(), head, &d, 1, &rec, ext, NSD_EXT_WORDS(NSD_EXT_MAX_LAYERS),
						   &big_ts, fed);
		if (rc == NSD_OK) {
			if (timed && big_ts > now)
				now = big_ts;
			rc = after(++fed, now);
		}
	}
	nsd_pcap_close(p);
	return rc == NSD_OK ? (long)fed : rc;
}
} // namespace

extern "C" long nsd_pcap_flows(const char *path, int mode, const nsd_bpf_prog *filter, nsd_flow_table *t)
{
	return pcap_flows_loop(path, mode, filter, t, FLOWS_MAX_N, [](uint64_t, uint64_t) { return (long)NSD_OK; });
}

// The same loop with idle flows leaving between the batches (the header's
// "flow expiry"): once more than `idle` packets are fed, the flows whose last
// packet lies more than `idle` packets back go to `sink`, sorted by `first`.
extern "C" long nsd_pcap_flows_expire(const char *path, int mode, const nsd_bpf_prog *filter, nsd_flow_table *t,
				      uint32_t every, uint64_t idle, uint32_t flags, nsd_flow_sink sink, void *user)
{
	if (!sink || (flags & ~NSD_FLOW_EXPIRE_PAIRED))
		return NSD_ERR_ARG;
	std::vector<nsd_flow> rows;
	return pcap_flows_loop(path, mode, filter, t, every, [&](uint64_t fed, uint64_t) -> long {
		if (fed <= idle)
			return NSD_OK;
		const long q = nsd_flow_expire_rows(t, fed - idle, flags, UINT32_MAX, rows, nullptr);
		if (q < 0)
			return q;
		if (!rows.empty() && sink(rows.data(), (uint32_t)rows.size(), user) != 0)
			return NSD_ERR_ARG;
		return NSD_OK;
	});
}

// The same by time (the header's "flow times"): once the largest timestamp
// fed exceeds idle_ns, the flows whose t_last lies more than idle_ns before it
// go to `sink` with their times, sorted by `first`.
extern "C" long nsd_pcap_flows_expire_ts(const char *path, int mode, const nsd_bpf_prog *filter, nsd_flow_table *t,
					 uint32_t every, uint64_t idle_ns, uint32_t flags, nsd_flow_sink_ts sink,
					 void *user)
{
	if (!sink || (flags & ~NSD_FLOW_EXPIRE_PAIRED) || !nsd_flow_is_timed(t))
		return NSD_ERR_ARG;
	std::vector<nsd_flowt> rows;
	return pcap_flows_loop(path, mode, filter, t, every, [&](uint64_t, uint64_t now) -> long {
		if (now <= idle_ns)
			return NSD_OK;
		const long q = nsd_flow_expire_rows_ts(t, now - idle_ns, flags, UINT32_MAX, rows, nullptr);
		if (q < 0)
			return q;
		if (!rows.empty() && sink(rows.data(), (uint32_t)rows.size(), user) != 0)
			return NSD_ERR_ARG;
		return NSD_OK;
	});
}

// The replay's staging: pinned host buffers per batch slot and the device pipe.
namespace {
constexpr uint32_t BATCH = 1u << 16;
constexpr size_t FRAME_BYTES = 32ull << 20;
constexpr int DEPTH = 3;           // batches on the device
constexpr int NSLOT = DEPTH + 4;   // + being copied, being rendered, rendered, being written
// the side words and room for a quarter of a batch to take a deep (> 12
// layer) entry; a chain the pool cannot hold is rendered per packet
constexpr uint32_t EXT_WORDS = BATCH + BATCH / 4 * NSD_EXT_WORDS(NSD_EXT_MAX_LAYERS);

// one formatter part's text: a cache line of its own, as every append writes
// the string's length (adjacent std::strings shared lines between the pool's
// threads: per-packet false sharing that cost the 16-thread pool 3x per record)
struct alignas(64) TextPart {
	std::string s;
};

struct ReplayRes {
	nsd_pipe *pipe = nullptr;
	struct {
		uint8_t *frames;
		nsd_desc_t *desc;
		nsd_sll_t *sll;
		nsd_crec *rec;
		uint32_t *ext;
	} buf[NSLOT] = {};
	// each record's frame header fields (show_frame_hdr)
	std::vector<nsd_frame_hdr_t> fh[NSLOT];
	// a mapped file's record offsets (scan_batch)
	std::vector<uint64_t> src[NSLOT];
	// the formatter parts' text buffers per slot, kept with their capacity:
	// regrown per replay they faulted in hundreds of MB of fresh pages,
	// with the formatter threads queued on the page-table lock
	std::vector<TextPart> part[NSLOT];
	bool ready() const { return pipe != nullptr; }
	long create(int lt, int mode)
	{
		pipe = nsd_pipe_create_compact(BATCH, FRAME_BYTES, EXT_WORDS, DEPTH, lt, mode);
		if (!pipe)
			return NSD_ERR_HIP;
		for (auto &x : buf) {
			x.frames = (uint8_t *)nsd_host_alloc(FRAME_BYTES);
			x.desc = (nsd_desc_t *)nsd_host_alloc(BATCH * sizeof(nsd_desc_t));
			x.sll = (nsd_sll_t *)nsd_host_alloc(BATCH * sizeof(nsd_sll_t));
			x.rec = (nsd_crec *)nsd_host_alloc(BATCH * sizeof(nsd_crec));
			x.ext = (uint32_t *)nsd_host_alloc(EXT_WORDS * sizeof(uint32_t));
			if (!x.frames || !x.desc || !x.sll || !x.rec || !x.ext) {
				release();
				return NSD_ERR_NOMEM;
			}
		}
		for (auto &v : fh)
			v.resize(BATCH);
		for (auto &v : src)
			v.resize(BATCH);
		return NSD_OK;
	}
	void release()
	{
		for (auto &x : buf) {
			nsd_host_free(x.frames);
			nsd_host_free(x.desc);
			nsd_host_free(x.sll);
			nsd_host_free(x.rec);
			nsd_host_free(x.ext);
			x = {};
		}
		for (auto &v : part)
			std::vector<TextPart>().swap(v);
		for (auto &v : fh)
			std::vector<nsd_frame_hdr_t>().swap(v);
		for (auto &v : src)
			std::vector<uint64_t>().swap(v);
		nsd_pipe_destroy(pipe);
		pipe = nullptr;
	}
};
std::mutex g_replay_mu;
ReplayRes g_replay;

// The CPUs the formatter pool runs on: one per physical core (an SMT
// sibling formats at a fraction of a core's rate), those of the calling
// thread's NUMA node first, of the CPUs this process may use.  Empty when
// the topology cannot be read (then nothing is pinned), or NSD_REPLAY_PIN=0.
// The topology is read from /sys once per process.
struct CpuTopo {
	int cpu;
	long pkg, core;
	int node;
};
const std::vector<CpuTopo> &cpu_topology()
{
	static const std::vector<CpuTopo> topo = [] {
		std::vector<CpuTopo> t;
		auto rd = [](int cpu, const char *what) -> long {
			char path[128];
			snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/%s", cpu, what);
			FILE *f = fopen(path, "r");
			if (!f)
				return -1;
			long v = -1;
			if (fscanf(f, "%ld", &v) != 1)
				v = -1;
			fclose(f);
			return v;
		};
		for (int c = 0; c < CPU_SETSIZE; c++) {
			const long pkg = rd(c, "topology/physical_package_id"), core = rd(c, "topology/core_id");
			if (pkg < 0 || core < 0)
				continue;
			int node = 0;
			for (int n = 0; n < 64; n++) {
				char path[128];
				snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/node%d", c, n);
				if (access(path, F_OK) == 0) {
					node = n;
					break;
				}
			}
			t.push_back({ c, pkg, core, node });
		}
		return t;
	}();
	return topo;
}

std::vector<int> pool_cpus()
{
	std::vector<int> out;
	const char *e = getenv("NSD_REPLAY_PIN");
	if (e && e[0] == '0')
		return out;
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) != 0)
		return out;
	const std::vector<CpuTopo> &topo = cpu_topology();
	const int me = sched_getcpu();
	const CpuTopo *mine = nullptr;
	for (const CpuTopo &t : topo)
		if (t.cpu == me)
			mine = &t;
	std::vector<std::pair<long, long>> seen;   // (package, core)
	std::vector<int> near, far;
	int first = -1;                            // the caller's core
	for (const CpuTopo &t : topo) {
		if (!CPU_ISSET(t.cpu, &set))
			continue;
		bool dup = false;
		for (auto &x : seen)
			dup = dup || (x.first == t.pkg && x.second == t.core);
		if (dup)
			continue;
		seen.emplace_back(t.pkg, t.core);
		if (mine && t.pkg == mine->pkg && t.core == mine->core)
			first = t.cpu;
		else
			(!mine || t.node == mine->node ? near : far).push_back(t.cpu);
	}
	// the caller's core first (the pool leaves it to the reader)
	if (first >= 0)
		out.push_back(first);
	out.insert(out.end(), near.begin(), near.end());
	out.insert(out.end(), far.begin(), far.end());
	return out;
}

// Stage times of one replay, printed to stderr when NSD_REPLAY_STATS is set
// in the environment (the pipeline's balance on a given host): the reader,
// the device waits, the formatter jobs (summed over the pool), the writer,
// and the reader's waits for a free slot.
struct ReplayStats {
	std::atomic<uint64_t> read{ 0 }, scan{ 0 }, ix{ 0 }, dev{ 0 }, fmt{ 0 }, write{ 0 }, slot{ 0 }, jobs{ 0 };
	static uint64_t now()
	{
		return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
			       std::chrono::steady_clock::now().time_since_epoch())
			.count();
	}
};

// one batch's buffers and its way through the stages
struct Slot {
	uint8_t *frames = nullptr;
	nsd_desc_t *desc = nullptr;
	nsd_sll_t *sll = nullptr;
	uint8_t *rhdr = nullptr;   // record headers as read (pcap write-out)
	nsd_frame_hdr_t *fh = nullptr;
	uint64_t *src = nullptr;   // record offsets in a mapped file
	int fill_left = 0;         // copy jobs of the batch not done (under mu)
	uint64_t count0 = 0;       // the packet counter of the batch's first record
	nsd_crec *rec = nullptr;
	uint32_t *ext = nullptr;
	uint32_t *verdict = nullptr;
	uint32_t ext_used = 0, n = 0;
	uint64_t cnt[NSD_NCOUNTERS];
	int status = 0;
	uint64_t seq = 0;
	int parts = 0, left = 0;   // render jobs, jobs not done (under mu)
	std::vector<TextPart> *part = nullptr;   // the ReplayRes's part[slot]
	long prc = NSD_OK;         // first render error (under mu)
};

// (slot, part, parts): render jobs, and the jobs of a mapped file's reader
// (copies of a batch, parts > 0; record index chunks, slot -1), which the
// pool takes first, in the order given
struct Job {
	int slot, part, parts;
};

// One replay.  Three stages run at once over a ring of batch slots (pinned
// host buffers):
//   - the calling thread (run) reads a batch, filters it and submits it to
//     the device pipe (compact records, DEPTH batches in flight); when the
//     pipe is full it completes the oldest batch and queues its render jobs;
//   - `threads` formatter threads (a pool for the whole replay) render the
//     batch's contiguous packet ranges, each into its own text buffer;
//   - a writer thread writes each batch's buffers in file order (writev, or
//     through the tprintf wrap when cols > 0), then the pcap write-out, and
//     frees the slot.
// So reading and walking batch k+1 overlap the rendering of batch k and the
// writing of batch k-1.  A record above NSD_MAX_CAPLEN waits for everything
// before it to be written, then goes through the per-packet path.
struct Replay {
	Replay(nsd_pcap *p, ReplayRes &res, int mode, const nsd_bpf_prog *filter, int out_fd, int cols,
	       uint64_t *counters, int threads, int pcap_fd);
	long run();

	// ---- fixed for the run (any thread reads them) ----
	nsd_pcap *const p;   // (the pool reads the mapped file; the reader's position is the reader thread's)
	nsd_pipe *const pipe;
	const int mode;
	const nsd_bpf_prog *const filter;
	const int out_fd, cols;
	const int threads, pcap_fd;
	const int lt;
	const bool ll_used;   // has_ll(p)
	const bool stats;     // NSD_REPLAY_STATS
	ReplayStats st;       // (atomics)
	const uint64_t t_start = ReplayStats::now();
	const std::vector<int> cpus = pool_cpus();
	std::vector<Slot> b;   // (a slot's fields are its current stage's; those marked are under mu)
	std::vector<uint32_t> verdicts;
	std::vector<uint8_t> rhdrs;
	std::mutex mu;
	std::condition_variable cv_job, cv_write, cv_free, cv_fill;

	// ---- under mu ----
	std::deque<Job> jobs, fills;
	std::vector<int> free_slots;
	std::deque<int> to_write;             // slots in file order, waiting for their render
	uint64_t next_seq = 0, written = 0;   // batches handed to the writer / written
	long err = NSD_OK;                    // first error of any stage
	bool stop = false;
	long printed = 0;                     // (and one_big, while the writer is idle)
	int ix_left = 0;                      // index chunk jobs not done

	// ---- reader thread only ----
	uint64_t *const counters;
	long rc = NSD_OK;
	uint64_t counted = 0;                 // read_pcap's ctx->tx_packets (netsniff-ng.c:730)
	std::deque<int> on_device;
	int pend = -1;                        // a mapped file's batch whose copy is on the pool
	long pend_n = 0;
	std::vector<uint8_t> big;             // a record above NSD_MAX_CAPLEN
	// the index window being built: written before its chunk jobs are queued,
	// read by the pool's chunk jobs, spliced after the join
	std::vector<size_t> ix_b;
	std::vector<IxChunk> ix_chunks;
	bool ix_flight = false;

	// ---- writer thread only (and one_big, while the writer is idle) ----
	long wrap_state = 0;
	std::string wrapped;

	// work pool
	void pool_thread(int t);
	void run_fill(std::unique_lock<std::mutex> &lk);
	template <class Pred> void help_until(Pred done);
	long render(Slot &x, int t);
	void start_fill(Slot &x, int k);
	void wait_fill(Slot &x) { help_until([&] { return x.fill_left <= 0; }); }
	// index-ahead of a mapped file
	void ix_launch(size_t start);
	void ix_join();
	void build_index();
	// writer
	void writer_thread();
	long put_text(const std::string &t);
	long put_parts(const Slot &x);
	long put_records(const Slot &x);
	// device stage
	long submit_slot(int k, long n);
	long complete_oldest();
	long flush_all();
	// reader loop
	int take_slot();
	void give_back(int slot);
	long read_into(int k, uint64_t t0);
	bool submit_pending(int k, long n);
	long one_big();
	void finish(std::vector<std::thread> &pool, std::thread &writer);
};

Replay::Replay(nsd_pcap *p_, ReplayRes &res, int mode_, const nsd_bpf_prog *filter_, int out_fd_, int cols_,
	       uint64_t *counters_, int threads_, int pcap_fd_)
	: p(p_), pipe(res.pipe), mode(mode_), filter(filter_), out_fd(out_fd_), cols(cols_), threads(threads_),
	  pcap_fd(pcap_fd_), lt((int)p_->linktype), ll_used(has_ll(p_)), stats(getenv("NSD_REPLAY_STATS") != nullptr),
	  b(NSLOT), verdicts(filter_ ? (size_t)NSLOT * BATCH : 0), rhdrs(pcap_fd_ >= 0 ? (size_t)NSLOT * BATCH * 32 : 0),
	  counters(counters_)
{
	for (int k = 0; k < NSLOT; k++) {
		Slot &x = b[k];
		x.frames = res.buf[k].frames;
		x.desc = res.buf[k].desc;
		x.rec = res.buf[k].rec;
		x.ext = res.buf[k].ext;
		x.sll = res.buf[k].sll;
		x.fh = res.fh[k].data();
		x.src = res.src[k].data();
		x.verdict = filter ? &verdicts[(size_t)k * BATCH] : nullptr;
		x.rhdr = pcap_fd >= 0 ? &rhdrs[(size_t)k * BATCH * 32] : nullptr;
		x.part = &res.part[k];
		if (x.part->size() < (size_t)threads)
			x.part->resize(threads);
	}
	for (int k = NSLOT - 1; k >= 0; k--)
		free_slots.push_back(k);
}

// ---- work pool ------------------------------------------------------------------
// part t of a slot = its packets [n t / parts, n (t+1) / parts)
long Replay::render(Slot &x, int t)
{
	const uint32_t lo = (uint32_t)((uint64_t)x.n * t / x.parts), hi = (uint32_t)((uint64_t)x.n * (t + 1) / x.parts);
	std::string &s = (*x.part)[t].s;
	s.clear();
	return nsd::format_replay_part(s, x.frames, x.desc, x.fh, x.sll, x.rec, x.ext, x.count0, lo, hi, lt, mode);
}

// the front job of `fills`, taken with mu held (returns with it held): copy
// job `part` of `parts` of a mapped file's batch, or an index chunk
void Replay::run_fill(std::unique_lock<std::mutex> &lk)
{
	const Job j = fills.front();
	fills.pop_front();
	lk.unlock();
	if (j.slot < 0) {
		ix_chunk(p, ix_b, j.part, ix_chunks[j.part]);
	} else {
		Slot &x = b[j.slot];
		const uint32_t lo = (uint32_t)((uint64_t)x.n * j.part / j.parts),
			       hi = (uint32_t)((uint64_t)x.n * (j.part + 1) / j.parts);
		fill_range(p, x.frames, x.desc, x.src, lo, hi, x.sll, x.fh, x.rhdr);
	}
	lk.lock();
	if (j.slot < 0 ? --ix_left == 0 : --b[j.slot].fill_left == 0)
		cv_fill.notify_all();
}

// the reader joins jobs it gave the pool: it takes the fill jobs still
// queued (in file order: its own or earlier ones) until done() holds
template <class Pred> void Replay::help_until(Pred done)
{
	std::unique_lock<std::mutex> lk(mu);
	while (!done()) {
		if (!fills.empty())
			run_fill(lk);
		else
			cv_fill.wait(lk);
	}
}

// the copy of a scanned batch (x.n records in slot k) goes to the pool while
// the reader scans the next batch; wait_fill joins it
void Replay::start_fill(Slot &x, int k)
{
	const int parts = x.n < 4096 ? 1 : (int)std::min<uint32_t>((uint32_t)threads + 1, x.n / 2048);
	std::lock_guard<std::mutex> g(mu);
	x.fill_left = parts;
	for (int q = 0; q < parts; q++)
		fills.push_back({ k, q, parts });
	cv_job.notify_all();
}

void Replay::pool_thread(int t)
{
	if (!cpus.empty()) {
		// one formatter per physical core, near the caller; the caller's own
		// core (the reader) is left out while others remain
		cpu_set_t one;
		CPU_ZERO(&one);
		const size_t k = cpus.size() > 1 ? 1 + (size_t)t % (cpus.size() - 1) : 0;
		CPU_SET(cpus[k], &one);
		(void)pthread_setaffinity_np(pthread_self(), sizeof(one), &one);
	}
	std::unique_lock<std::mutex> lk(mu);
	for (;;) {
		cv_job.wait(lk, [&] { return stop || !jobs.empty() || !fills.empty(); });
		if (jobs.empty() && fills.empty())
			return;
		if (!fills.empty()) {
			run_fill(lk);
			continue;
		}
		const Job j = jobs.front();
		jobs.pop_front();
		lk.unlock();
		const uint64_t t0 = stats ? ReplayStats::now() : 0;
		const long r = render(b[j.slot], j.part);
		if (stats) {
			st.fmt += ReplayStats::now() - t0;
			st.jobs++;
		}
		lk.lock();
		Slot &x = b[j.slot];
		if (r != NSD_OK && x.prc == NSD_OK)
			x.prc = r;
		if (--x.left == 0)
			cv_write.notify_all();
	}
}

// ---- index-ahead ----------------------------------------------------------------
// A mapped file's index windows: the chunks of the window after the one the
// reader scans run on the pool meanwhile (a window's start is the end of the
// one before, known once that one is spliced).
void Replay::ix_launch(size_t start)
{
	const int nc = threads + 1;
	ix_b = ix_bounds(p, start, ix_window(), nc);
	if ((int)ix_chunks.size() != nc)
		ix_chunks.resize(nc);
	std::lock_guard<std::mutex> g(mu);
	ix_left = nc;
	for (int c = 0; c < nc; c++)
		fills.push_back({ -1, c, nc });
	ix_flight = true;
	cv_job.notify_all();
}

void Replay::ix_join()
{
	help_until([&] { return ix_left <= 0; });
	ix_flight = false;
}

void Replay::build_index()
{
	if (!ix_flight)
		ix_launch(p->pos);
	ix_join();
	ix_splice(p, ix_b, ix_chunks);
	if (!p->ix_end)
		ix_launch(p->ix_off.empty() ? ix_b[0] : p->ix_off.back() + p->hdrsize + p->ix_cap.back());
}

// ---- writer ---------------------------------------------------------------------
// one piece of text to out_fd (wrapped when cols > 0)
long Replay::put_text(const std::string &t)
{
	if (cols > 0 && !t.empty()) {
		wrapped.resize(2 * t.size() + 16);
		const long k = nsd_tprintf_wrap(t.data(), t.size(), cols, &wrap_state, &wrapped[0], wrapped.size());
		if (k < 0)
			return k;
		return write_all(out_fd, wrapped.data(), (size_t)k) ? NSD_OK : NSD_ERR_ARG;
	}
	return write_all(out_fd, t.data(), t.size()) ? NSD_OK : NSD_ERR_ARG;
}

long Replay::put_parts(const Slot &x)
{
	if (cols > 0) {
		for (int t = 0; t < x.parts; t++) {
			const long r = put_text((*x.part)[t].s);
			if (r != NSD_OK)
				return r;
		}
		return NSD_OK;
	}
	std::vector<struct iovec> iov;
	for (int t = 0; t < x.parts; t++)
		if (!(*x.part)[t].s.empty())
			iov.push_back({ (void *)(*x.part)[t].s.data(), (*x.part)[t].s.size() });
	size_t k = 0;
	while (k < iov.size()) {
		const int cnt = (int)(iov.size() - k < 512 ? iov.size() - k : 512);
		ssize_t w = writev(out_fd, &iov[k], cnt);
		if (w < 0 && errno == EINTR)
			continue;
		if (w <= 0)
			return NSD_ERR_ARG;
		while (w > 0 && k < iov.size()) {   // advance past what was written
			if ((size_t)w >= iov[k].iov_len) {
				w -= (ssize_t)iov[k].iov_len;
				k++;
			} else {
				iov[k].iov_base = (uint8_t *)iov[k].iov_base + w;
				iov[k].iov_len -= (size_t)w;
				w = 0;
			}
		}
	}
	return NSD_OK;
}

// the `--out f.pcap` write-out of read_pcap (netsniff-ng.c:636, 693-697,
// 739-746): every record that passed the filter exactly as it was read
// (record header incl. the *_LL cooked header, then its bytes: write_pcap(fdo,
// &phdr, magic, out, pcap_get_length) of pcap_sg.c / pcap_rw.c), in file order
long Replay::put_records(const Slot &x)
{
	if (pcap_fd < 0)
		return NSD_OK;
	std::string recs;
	for (uint32_t k = 0; k < x.n; k++) {
		recs.append((const char *)x.rhdr + 32 * (size_t)k, p->hdrsize);
		recs.append((const char *)x.frames + NSD_DESC_OFF(x.desc[k]), NSD_DESC_CAPLEN(x.desc[k]));
	}
	return write_all(pcap_fd, recs.data(), recs.size()) ? NSD_OK : NSD_ERR_ARG;
}

// Batches leave in file order (to_write), each once its render jobs are done.
// The first error of any stage stays in err; after it nothing more is written,
// the slots still pass through so that every stage winds down.
void Replay::writer_thread()
{
	std::unique_lock<std::mutex> lk(mu);
	for (;;) {
		cv_write.wait(lk, [&] { return (!to_write.empty() && b[to_write.front()].left == 0) ||
					       (stop && to_write.empty()); });
		if (to_write.empty())
			return;
		const int k = to_write.front();
		to_write.pop_front();
		Slot &x = b[k];
		long r = x.prc;
		const bool skip = err != NSD_OK;
		lk.unlock();
		const uint64_t t0 = stats ? ReplayStats::now() : 0;
		if (!skip && r == NSD_OK)
			r = put_parts(x);
		if (!skip && r == NSD_OK)
			r = put_records(x);
		if (stats)
			st.write += ReplayStats::now() - t0;
		lk.lock();
		if (r != NSD_OK && err == NSD_OK)
			err = r;
		if (!skip && r == NSD_OK)
			printed += x.n;
		written++;
		free_slots.push_back(k);
		cv_free.notify_all();
	}
}

// ---- device stage -----------------------------------------------------------------
// slot k's n records read: filtered (bpf_run_filter per record before the
// dissector, netsniff-ng.c:723-725) and submitted to the device
long Replay::submit_slot(int k, long n)
{
	Slot &x = b[k];
	const size_t used = batch_extent(x.desc, (size_t)n);
	if (filter) {
		int r = nsd_bpf_filter_batch(filter, x.frames, used, x.desc, (uint32_t)n, x.verdict);
		if (r != NSD_OK) {
			give_back(k);
			return r;
		}
		long m = 0;
		for (long j = 0; j < n; j++)
			if (x.verdict[j]) {
				x.sll[m] = x.sll[j];
				x.fh[m] = x.fh[j];
				if (x.rhdr && m != j)
					memcpy(x.rhdr + 32 * (size_t)m, x.rhdr + 32 * (size_t)j, 32);
				x.desc[m++] = x.desc[j];
			}
		n = m;
		if (n == 0) {
			give_back(k);
			return NSD_OK;
		}
	}
	if ((int)on_device.size() == DEPTH)
		complete_oldest();
	x.n = (uint32_t)n;
	x.count0 = counted + 1;
	counted += x.n;
	x.status = NSD_OK;
	memset(x.cnt, 0, sizeof(x.cnt));
	int r = nsd_pipe_submit_compact(pipe, x.frames, used, x.desc, ll_used ? x.sll : nullptr, x.n, x.rec, x.ext,
					&x.ext_used, x.cnt, &x.status);
	if (r != NSD_OK) {
		give_back(k);
		return r;
	}
	on_device.push_back(k);
	return NSD_OK;
}

// the oldest device batch completed: to the writer's queue, its render jobs
// to the pool
long Replay::complete_oldest()
{
	const int k = on_device.front();
	on_device.pop_front();
	Slot &x = b[k];
	const uint64_t t0 = stats ? ReplayStats::now() : 0;
	const int ws = nsd_pipe_wait(pipe);
	if (stats)
		st.dev += ReplayStats::now() - t0;
	long r = ws != NSD_OK ? (ws < 0 ? ws : NSD_ERR_HIP) : x.status;
	if (r == NSD_OK && counters)
		for (int c = 0; c < NSD_NCOUNTERS; c++)
			counters[c] += x.cnt[c];
	std::lock_guard<std::mutex> g(mu);
	x.parts = x.n < 2048 ? 1 : threads;
	x.left = x.parts;
	x.prc = r;
	x.seq = next_seq++;
	to_write.push_back(k);
	if (r == NSD_OK) {
		for (int t = 0; t < x.parts; t++)
			jobs.push_back({ k, t, 0 });
		cv_job.notify_all();
	} else {
		x.left = 0;
		cv_write.notify_all();
	}
	return r;
}

// everything read so far through the device, rendered and written
long Replay::flush_all()
{
	while (!on_device.empty())
		complete_oldest();
	std::unique_lock<std::mutex> lk(mu);
	cv_free.wait(lk, [&] { return written == next_seq; });
	return err;
}

// ---- reader loop --------------------------------------------------------------------
void Replay::give_back(int slot)
{
	std::lock_guard<std::mutex> g(mu);
	free_slots.push_back(slot);
}

// a free slot (completing device batches while there is none), or -1 with rc
// set once a stage has failed
int Replay::take_slot()
{
	for (;;) {
		std::unique_lock<std::mutex> lk(mu);
		if (err != NSD_OK) {
			rc = err;
			return -1;
		}
		if (free_slots.empty()) {
			lk.unlock();
			if (!on_device.empty()) {
				complete_oldest();
				continue;
			}
			lk.lock();
			const uint64_t t0 = stats ? ReplayStats::now() : 0;
			cv_free.wait(lk, [&] { return !free_slots.empty(); });
			if (stats)
				st.slot += ReplayStats::now() - t0;
		}
		const int k = free_slots.back();
		free_slots.pop_back();
		return k;
	}
}

// the next batch into slot k: read, or for a mapped file scanned (its copy
// started on the pool); the records, 0 at the end, or a negative NSD_ERR_*
long Replay::read_into(int k, uint64_t t0)
{
	Slot &x = b[k];
	if (!p->map)
		return read_batch(p, x.frames, FRAME_BYTES, x.desc, x.sll, x.fh, BATCH, nullptr, nullptr, x.rhdr);
	size_t end = 0;
	if (ix_need(p)) {
		build_index();
		if (stats)
			st.ix += ReplayStats::now() - t0;
	}
	const long n = scan_batch(p, FRAME_BYTES, x.desc, x.src, BATCH, &end);
	if (stats)
		st.scan += ReplayStats::now() - t0;
	if (n > 0) {
		x.n = (uint32_t)n;
		memset(x.frames + end, 0, NSD_FRAME_PAD);
		start_fill(x, k);
	}
	return n;
}

// the mapped batch before the one just scanned into slot k (n): its copy
// done, on to the device (file order).  false: it failed, rc is set and slot
// k is given back
bool Replay::submit_pending(int k, long n)
{
	if (pend < 0)
		return true;
	const int j = pend;
	pend = -1;
	wait_fill(b[j]);
	const long r = submit_slot(j, pend_n);
	if (r == NSD_OK)
		return true;
	if (n > 0 && p->map)
		wait_fill(b[k]);
	give_back(k);
	rc = r;
	return false;
}

// a record longer than a batch can carry: after the batches before it,
// filtered and dissected on its own through the per-packet path
long Replay::one_big()
{
	long r = flush_all();
	if (r != NSD_OK)
		return r;
	nsd_sll_t ll;
	nsd_frame_hdr_t fh;
	uint8_t hdr[32];
	bool pass;
	const long caplen = read_big(p, filter, big, &ll, &fh, hdr, &pass);
	if (caplen <= 0 || !pass)
		return caplen < 0 ? caplen : NSD_OK;
	if (counters)
		nsd::cpu_count_packet(big.data(), (uint32_t)caplen, lt, mode, ll_used ? &ll : nullptr, counters);
	std::string text;
	nsd::format_frame_hdr(text, fh, &ll, big.data(), (uint32_t)caplen, lt, mode, ++counted);
	r = nsd::render_packet_cpu(text, big.data(), (size_t)caplen, lt, mode, &ll);
	if (r != NSD_OK)
		return r;
	// (the writer is idle: every batch before this record is written)
	r = put_text(text);
	if (r == NSD_OK && pcap_fd >= 0 &&
	    !(write_all(pcap_fd, hdr, p->hdrsize) && write_all(pcap_fd, big.data(), (size_t)caplen)))
		r = NSD_ERR_ARG;
	if (r == NSD_OK)
		printed++;
	return r;
}

// the reader has stopped (the end of the file, or an error): what it left
// drains, then the threads go
void Replay::finish(std::vector<std::thread> &pool, std::thread &writer)
{
	if (ix_flight)
		ix_join();   // (an index window no scan reached)
	if (pend >= 0) {
		// (left by an error: its copy drains before the slots go away)
		wait_fill(b[pend]);
		give_back(pend);
	}
	const long r = flush_all();
	if (rc == NSD_OK)
		rc = r;
	{
		std::lock_guard<std::mutex> g(mu);
		stop = true;
	}
	cv_job.notify_all();
	cv_write.notify_all();
	for (auto &t : pool)
		t.join();
	writer.join();
	if (stats)
		fprintf(stderr,
			"nsd_replay: %ld records, %d threads, %.1f ms: read %.1f (scan %.1f, index %.1f), device waits %.1f, slot waits %.1f, "
			"format %.1f (%llu jobs, %.1f per thread), write %.1f ms\n",
			printed, threads, (ReplayStats::now() - t_start) / 1e6, st.read / 1e6, st.scan / 1e6, st.ix / 1e6, st.dev / 1e6, st.slot / 1e6,
			st.fmt / 1e6, (unsigned long long)st.jobs.load(), st.fmt / 1e6 / threads, st.write / 1e6);
}

// the records printed, or a negative NSD_ERR_*
long Replay::run()
{
	std::vector<std::thread> pool;
	for (int t = 0; t < threads; t++)
		pool.emplace_back([this, t] { pool_thread(t); });
	std::thread writer([this] { writer_thread(); });
	while (rc == NSD_OK) {
		const int k = take_slot();
		if (k < 0)
			break;
		const uint64_t tr = stats ? ReplayStats::now() : 0;
		const long n = read_into(k, tr);
		if (!submit_pending(k, n))
			break;
		if (stats)
			st.read += ReplayStats::now() - tr;
		if (n == NSD_ERR_CAPLEN) {
			give_back(k);
			rc = one_big();
		} else if (n <= 0) {
			give_back(k);
			if (n < 0)
				rc = n;
			break;
		} else if (p->map) {
			pend = k;
			pend_n = n;
		} else {
			rc = submit_slot(k, n);
		}
	}
	finish(pool, writer);
	return rc == NSD_OK ? printed : rc;
}

} // namespace

// The replay loop: read -> [BPF filter on the device] -> device walk (pipelined,
// `depth` batches in flight) -> host formatter -> [tprintf wrap] -> out_fd.
// Writes the text dissector_entry_point prints for each accepted record, in
// file order.  `filter` may be NULL (every record passes, bpf.c:711).
// `cols` > 0 wraps like tprintf at that width, 0 writes the unwrapped stream.
// counters (may be NULL) accumulates the per-protocol counter vector.
// `threads` host threads render each batch (<= 0: up to 16 by the hardware).
// Returns the records printed, or a negative NSD_ERR_*.
extern "C" long nsd_replay_pcap(const char *path, int mode, const nsd_bpf_prog *filter, int out_fd,
				int cols, uint64_t *counters, int threads)
{
	return nsd_replay_pcap_out(path, mode, filter, out_fd, cols, counters, threads, -1);
}

// As nsd_replay_pcap; with pcap_fd >= 0 also the `--out f.pcap` write-out
// of read_pcap: the file header, then every record that passed the filter
// exactly as it was read, in file order (Replay::put_records).
extern "C" long nsd_replay_pcap_out(const char *path, int mode, const nsd_bpf_prog *filter, int out_fd,
				    int cols, uint64_t *counters, int threads, int pcap_fd)
{
	if (threads <= 0) {
		const unsigned hc = std::thread::hardware_concurrency();
		threads = hc ? (int)(hc < 16 ? hc : 16) : 1;
	}
	if (threads > 64)
		threads = 64;
	nsd_pcap *p = nsd_pcap_open(path);
	if (!p)
		return NSD_ERR_ARG;
	nsd_if_cache_reset();   // interface names as they are now (renames since an earlier replay)
	const int lt = (int)p->linktype;
	if (pcap_fd >= 0 && !push_fhdr(p, pcap_fd)) {
		nsd_pcap_close(p);
		return NSD_ERR_ARG;
	}
	// the pinned staging and the device pipe (hundreds of MB: their set-up
	// costs about as much as replaying a million records) are kept for the
	// process and reused by the next replay; a replay running beside another
	// gets its own
	std::unique_lock<std::mutex> cache_lk(g_replay_mu, std::try_to_lock);
	ReplayRes own;
	ReplayRes &res = cache_lk.owns_lock() ? g_replay : own;
	long rc = res.ready() ? (long)nsd_pipe_retarget(res.pipe, lt, mode) : (long)res.create(lt, mode);
	if (rc == 1) {
		// the cached set was made on another device than the current one
		res.release();
		rc = res.create(lt, mode);
	}
	if (rc != NSD_OK) {
		nsd_pcap_close(p);
		return rc;
	}
	rc = Replay(p, res, mode, filter, out_fd, cols, counters, threads, pcap_fd).run();
	// (an error leaves batches in the pipe: drop the cached set then)
	if (&res == &own || rc < 0)
		res.release();
	nsd_pcap_close(p);
	return rc;
}

// dissector_cleanup_all (nsd_proto.cpp) frees the replay's cached buffers
extern "C" void nsd_replay_release(void)
{
	std::lock_guard<std::mutex> g(g_replay_mu);
	g_replay.release();
}
