// nsd_pcap_reader.h - the capture-file reader (nsd_pcap.cpp) as its drivers
// see it (nsd_replay.cpp: the replay and the flow table's file loop): the
// reader's state and the calls that are not part of the ABI.
#ifndef NSD_PCAP_READER_H
#define NSD_PCAP_READER_H

#include <errno.h>
#include <string.h>
#include <unistd.h>

#include <vector>

#include "nsd_internal.h"

struct nsd_pcap {
	int fd = -1;
	bool swapped = false;
	uint32_t hdrsize = 16;   // record header bytes (pcap_get_hdr_length)
	uint32_t ll_extra = 0;   // cooked-header bytes counted in caplen (*_LL)
	uint32_t linktype = 0;   // as stored in the file header
	uint32_t magic_raw = 0;  // as stored in the file header
	uint32_t magic = 0;      // in host order
	bool nsec = false;
	bool eof = false;
	// buffered reader (the scatter-gather reader's iovecs, pcap_sg.c), or a
	// regular file mapped whole (pcap_mm.c's way; the replay's reader then
	// only scans the record headers and the pool copies the bodies)
	std::vector<uint8_t> buf;
	const uint8_t *map = nullptr;
	size_t pos = 0, len = 0;
	// a mapped file's record index, one window at a time (IxChunk below):
	// the records' header offsets and caplens, ix_i the next one; ix_end =
	// the walk ended inside the indexed window (no records past the last)
	std::vector<uint64_t> ix_off;
	std::vector<uint32_t> ix_cap;
	size_t ix_i = 0;
	bool ix_end = false;

	const uint8_t *data() const { return map ? map : buf.data(); }
	bool fill(size_t need)
	{
		if (len - pos >= need)
			return true;
		if (map)
			return false;
		if (pos) {
			memmove(buf.data(), buf.data() + pos, len - pos);
			len -= pos;
			pos = 0;
		}
		if (buf.size() < need)
			buf.resize(need);
		while (len < need) {
			ssize_t r = read(fd, buf.data() + len, buf.size() - len);
			if (r < 0 && errno == EINTR)
				continue;
			if (r <= 0)
				return false;
			len += (size_t)r;
		}
		return true;
	}
};

namespace nsd {
namespace NSD_HIDDEN reader {

// one chunk of an index window, walked on its own (nsd_pcap.cpp)
struct IxChunk {
	std::vector<uint64_t> off;
	std::vector<uint32_t> cap;
	size_t next = 0;     // where the walk stopped (its last record's end)
	bool ended = false;  // stopped by the end rule, not at the chunk's end
};

// the dissector's SLL head reads the sockaddr_ll: an *_LL file's cooked
// headers, or a Kuznetzov / Borkmann file of an SLL link type (the frame
// headers read it for every file)
bool has_ll(const nsd_pcap *p);

// rhdr (may be NULL): each record's header bytes as stored (hdrsize <= 32,
// 32-byte stride), for the pcap write-out
long read_batch(nsd_pcap *p, uint8_t *frames, size_t cap, nsd_desc_t *desc, nsd_sll_t *sll, nsd_frame_hdr_t *fh,
		uint32_t max_n, uint32_t *wire_len, uint64_t *ts_ns, uint8_t *rhdr);
long read_one(nsd_pcap *p, std::vector<uint8_t> &frame, nsd_sll_t *sll, nsd_frame_hdr_t *fh, uint8_t *rhdr);

// a mapped file: the next batch's layout, then the copy of a range of it
long scan_batch(nsd_pcap *p, size_t cap, nsd_desc_t *desc, uint64_t *src, uint32_t max_n, size_t *end);
void fill_range(const nsd_pcap *p, uint8_t *frames, const nsd_desc_t *desc, const uint64_t *src, uint32_t lo,
		uint32_t hi, nsd_sll_t *sll, nsd_frame_hdr_t *fh, uint8_t *rhdr);

// a mapped file's record index: a window's chunk bounds, a chunk's walk (any
// thread, any order), the splice of the chunks into p's index
bool ix_need(const nsd_pcap *p);
size_t ix_window();
std::vector<size_t> ix_bounds(const nsd_pcap *p, size_t start, size_t window, int nc);
void ix_chunk(const nsd_pcap *p, const std::vector<size_t> &b, int c, IxChunk &out);
void ix_splice(nsd_pcap *p, const std::vector<size_t> &b, std::vector<IxChunk> &ch);

} // namespace reader
} // namespace nsd

#endif
