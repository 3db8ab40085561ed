// nsd_pcap.cpp - the pcap replay front end of the dissector path
// (`netsniff-ng --in file.pcap`, read_pcap netsniff-ng.c:640-770): a pcap
// reader that packs records into batches (frames + nsd_desc_t).  Its drivers
// are in nsd_replay.cpp (the replay, the flow table's file loop), which see
// it through nsd_pcap_reader.h.
//
// Reader semantics follow pcap_io.h and pcap_sg.c:
//   - file header validation and the *_LL remap for SLL / netlink files
//     (pcap_validate_header, pcap_io.h:874-908); the link type handed to the
//     dissector is the header field as stored, so a byte-swapped file passes
//     a byte-swapped link type (pcap_generic_pull_fhdr :910-928), which the
//     entry point matches either way (dissector.c:79);
//   - record header sizes per format (pcap_get_hdr_length :429-452: 16 for
//     usec / nsec, 32 for the *_LL forms whose 16-byte cooked header is not
//     packet data, 24 for the Kuznetzov / Borkmann forms), the caplen field
//     byte-swapped for swapped files and minus 16 for *_LL
//     (pcap_get_length :322-352);
//   - a record with caplen 0 or above the 1 MiB replay buffer ends the
//     replay, as pcap_sg_read's -EINVAL does (pcap_sg.c:121-123), and so
//     does a short read at the end of the file;
//   - a record longer than a batch can carry (NSD_MAX_CAPLEN < caplen <=
//     1 MiB: tcpdump's default snaplen is 262144, GRO frames are long) ends
//     the batch before it; the batch reader reports NSD_ERR_CAPLEN when it
//     is the next record, and the replay dissects it through the per-packet
//     path (nsd_proto.cpp), in file order.
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <sys/mman.h>
#include <sys/stat.h>

#include <algorithm>
#include <vector>

#include "nsd_pcap_reader.h"

using namespace nsd::reader;

namespace {

constexpr uint32_t TCPDUMP = 0xa1b2c3d4, NSEC = 0xa1b23c4d, KUZ = 0xa1b2cd34, BKM = 0xa1e2cb12;
constexpr uint32_t LT_LINUX_SLL = 113, LT_NETLINK = 253;
constexpr uint32_t REPLAY_BUF = 1024 * 1024;   // read_pcap's `out` buffer (netsniff-ng.c:680)

uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
uint16_t bswap16(uint16_t v) { return __builtin_bswap16(v); }

} // namespace

bool nsd::reader::has_ll(const nsd_pcap *p)
{
	return p->ll_extra != 0 || p->linktype == LT_LINUX_SLL || p->linktype == bswap32(LT_LINUX_SLL);
}

extern "C" nsd_pcap *nsd_pcap_open(const char *path)
{
	if (!path)
		return nullptr;
	int fd = open(path, O_RDONLY);
	if (fd < 0)
		return nullptr;
	nsd_pcap *p = new nsd_pcap;
	p->fd = fd;
	struct stat sb;
	const char *mm = getenv("NSD_PCAP_MMAP");
	if (!(mm && mm[0] == '0') && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size >= 24) {
		void *m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
		if (m != MAP_FAILED) {
			(void)madvise(m, (size_t)sb.st_size, MADV_SEQUENTIAL);
			p->map = (const uint8_t *)m;
			p->len = (size_t)sb.st_size;
		}
	}
	if (!p->map)
		p->buf.resize(4 << 20);
	uint8_t h[24];
	if (!p->fill(24)) {
		nsd_pcap_close(p);
		return nullptr;
	}
	memcpy(h, p->data(), 24);
	p->pos = 24;
	uint32_t magic, lt;
	memcpy(&magic, h, 4);
	memcpy(&lt, h + 20, 4);
	uint16_t vmaj, vmin;
	memcpy(&vmaj, h + 4, 2);
	memcpy(&vmin, h + 6, 2);
	// pcap_check_magic (pcap_io.h:286-320)
	p->magic_raw = magic;
	uint32_t m = magic;
	if (m == bswap32(TCPDUMP) || m == bswap32(NSEC) || m == bswap32(KUZ) || m == bswap32(BKM)) {
		p->swapped = true;
		m = bswap32(m);
	}
	if (m != TCPDUMP && m != NSEC && m != KUZ && m != BKM) {
		nsd_pcap_close(p);
		return nullptr;
	}
	// pcap_validate_header: version 2.4 in either byte order
	if ((vmaj != 2 && bswap16(vmaj) != 2) || (vmin != 4 && bswap16(vmin) != 4)) {
		nsd_pcap_close(p);
		return nullptr;
	}
	const uint32_t lt_host = p->swapped ? bswap32(lt) : lt;
	p->linktype = lt;
	p->magic = m;
	p->nsec = m == NSEC || m == BKM;
	if (m == KUZ || m == BKM) {
		p->hdrsize = 24;
	} else if (lt_host == LT_LINUX_SLL || lt_host == LT_NETLINK) {
		p->hdrsize = 32;   // *_LL: the cooked header follows the record header
		p->ll_extra = 16;
	}
	return p;
}

extern "C" int nsd_pcap_linktype(const nsd_pcap *p) { return p ? (int)p->linktype : -1; }

extern "C" void nsd_pcap_close(nsd_pcap *p)
{
	if (!p)
		return;
	if (p->map)
		munmap((void *)p->map, p->len);
	if (p->fd >= 0)
		close(p->fd);
	delete p;
}

// Read up to max_n records into frames[0, cap): frames packed at 16-byte
// aligned offsets (TPACKET_ALIGNMENT, as in the RX ring), NSD_FRAME_PAD bytes
// kept free past the last one.  desc[k] = NSD_DESC(offset, caplen);
// wire_len[k] (may be NULL) = the record's original length, ts_ns[k] (may be
// NULL) = its timestamp in ns.  Returns the records read (0 at the end of the
// replay), or NSD_ERR_ARG.
extern "C" long nsd_pcap_read_batch(nsd_pcap *p, uint8_t *frames, size_t cap, nsd_desc_t *desc,
				    uint32_t max_n, uint32_t *wire_len, uint64_t *ts_ns)
{
	return nsd_pcap_read_batch_sll(p, frames, cap, desc, nullptr, max_n, wire_len, ts_ns);
}

// What read_pcap's pcap_pkthdr_to_tpacket_hdr (pcap_io.h:594-709) makes of
// one record header h (as stored) in its frame_map, zeroed once
// (netsniff-ng.c:672) and overwritten field by field per record:
//   tp_sec = ts.tv_sec; tp_nsec = tv_usec * 1000 (usec, *_LL, Kuznetzov) or
//   the ns field (nsec, Borkmann); tp_len = len, minus the cooked header for
//   *_LL; all byte-swapped for swapped files (the usec product in 32 bits);
//   sll: the cooked header (*_LL: ll_to_sockaddr, pcap_io.h:182-191:
//   pkttype / hatype / halen from be16, protocol as stored, addr), or the
//   Kuznetzov ifindex / protocol / pkttype, or the Borkmann ifindex (u16) /
//   protocol / hatype / pkttype; every other field stays 0.
static void record_meta(const nsd_pcap *p, const uint8_t *h, nsd_sll_t *sll, nsd_frame_hdr_t *fh)
{
	const bool sw = p->swapped;
	auto r32 = [&](int o) { uint32_t v; memcpy(&v, h + o, 4); return sw ? bswap32(v) : v; };
	auto r16 = [&](int o) { uint16_t v; memcpy(&v, h + o, 2); return sw ? bswap16(v) : v; };
	if (fh) {
		memset(fh, 0, sizeof(*fh));
		fh->sec = r32(0);
		const uint32_t frac = r32(4);
		fh->nsec = p->nsec ? frac : frac * 1000u;
		fh->len = r32(12) - p->ll_extra;
	}
	if (!sll)
		return;
	nsd_sll_t ll;
	memset(&ll, 0, sizeof(ll));
	if (p->ll_extra) {
		const uint8_t *c = h + 16;   // struct pcap_ll, big-endian fields
		ll.pkttype = (uint8_t)(((uint32_t)c[0] << 8) | c[1]);
		ll.hatype = (uint16_t)(((uint32_t)c[2] << 8) | c[3]);
		ll.halen = (uint8_t)(((uint32_t)c[4] << 8) | c[5]);
		memcpy(ll.addr, c + 6, 8);
		memcpy(&ll.protocol, c + 14, 2);
	} else if (p->magic == KUZ) {
		// struct pcap_pkthdr_kuz {ts, caplen, len, u32 ifindex, u16 protocol, u8 pkttype}
		ll.ifindex = (int32_t)r32(16);
		ll.protocol = r16(20);
		ll.pkttype = h[22];
	} else if (p->magic == BKM) {
		// struct pcap_pkthdr_bkm {ts, caplen, len, u16 tsource, u16 ifindex,
		// u16 protocol, u8 hatype, u8 pkttype}
		ll.ifindex = r16(18);
		ll.protocol = r16(20);
		ll.hatype = h[22];
		ll.pkttype = h[23];
	}
	*sll = ll;
}

// same, also filling sll[k] (may be NULL) the way read_pcap fills fm.s_ll
// (netsniff-ng.c:672, 727): zeroed once, then for *_LL records
// pcap_pkthdr_to_tpacket_hdr -> ll_to_sockaddr (pcap_io.h:182-191, 594-660)
// from the cooked header after the record header (struct pcap_ll
// {pkttype, hatype, len, addr[8], protocol}, every field big-endian in either
// file byte order): pkttype / hatype / halen from be16, protocol kept as
// stored (be16), addr copied; family and ifindex stay 0.
extern "C" long nsd_pcap_read_batch_sll(nsd_pcap *p, uint8_t *frames, size_t cap, nsd_desc_t *desc,
					nsd_sll_t *sll, uint32_t max_n, uint32_t *wire_len, uint64_t *ts_ns)
{
	return read_batch(p, frames, cap, desc, sll, nullptr, max_n, wire_len, ts_ns, nullptr);
}

extern "C" long nsd_pcap_read_batch_fh(nsd_pcap *p, uint8_t *frames, size_t cap, nsd_desc_t *desc,
				       nsd_sll_t *sll, nsd_frame_hdr_t *fh, uint32_t max_n)
{
	return read_batch(p, frames, cap, desc, sll, fh, max_n, nullptr, nullptr, nullptr);
}

// rhdr (may be NULL): each record's header bytes as stored (hdrsize <= 32,
// 32-byte stride), for the pcap write-out
long nsd::reader::read_batch(nsd_pcap *p, uint8_t *frames, size_t cap, nsd_desc_t *desc, nsd_sll_t *sll,
			     nsd_frame_hdr_t *fh, uint32_t max_n, uint32_t *wire_len, uint64_t *ts_ns, uint8_t *rhdr)
{
	if (!p || !frames || !desc || cap < NSD_FRAME_PAD)
		return NSD_ERR_ARG;
	size_t off = 0;
	uint32_t n = 0;
	while (n < max_n && !p->eof) {
		if (!p->fill(p->hdrsize)) {
			p->eof = true;
			break;
		}
		const uint8_t *h = p->data() + p->pos;
		uint32_t sec, frac, cl, wl;
		memcpy(&sec, h, 4);
		memcpy(&frac, h + 4, 4);
		memcpy(&cl, h + 8, 4);
		memcpy(&wl, h + 12, 4);
		if (p->swapped) {
			sec = bswap32(sec);
			frac = bswap32(frac);
			cl = bswap32(cl);
			wl = bswap32(wl);
		}
		const uint32_t caplen = cl - p->ll_extra;   // unsigned, as the reference computes it
		if (caplen == 0 || caplen > REPLAY_BUF) {
			p->eof = true;   // pcap_sg_read: -EINVAL ends read_pcap's loop
			break;
		}
		if (caplen > NSD_MAX_CAPLEN) {
			if (n == 0)
				return NSD_ERR_CAPLEN;   // the next record does not fit a batch
			break;
		}
		const size_t at = (off + 15) & ~(size_t)15;
		if (at + caplen + NSD_FRAME_PAD > cap) {
			if (n == 0)
				return NSD_ERR_ARG;   // one record does not fit the batch buffer
			break;                        // next batch
		}
		if (!p->fill((size_t)p->hdrsize + caplen)) {
			p->eof = true;
			break;
		}
		h = p->data() + p->pos;
		memcpy(frames + at, h + p->hdrsize, caplen);
		p->pos += p->hdrsize + caplen;
		desc[n] = NSD_DESC(at, caplen);
		if (rhdr)
			memcpy(rhdr + 32 * (size_t)n, h, p->hdrsize);
		if (sll || fh)
			record_meta(p, h, sll ? sll + n : nullptr, fh ? fh + n : nullptr);
		if (wire_len)
			wire_len[n] = wl;
		if (ts_ns)
			ts_ns[n] = (uint64_t)sec * 1000000000ull + (p->nsec ? frac : (uint64_t)frac * 1000ull);
		off = at + caplen;
		n++;
	}
	memset(frames + off, 0, NSD_FRAME_PAD);
	return n;
}

// A mapped file's next batch, as read_batch lays it out (same checks, same
// stops), without touching the bodies: desc[k] = the record's place in the
// batch buffer, src[k] = its header's offset in the file.  fill_range copies
// a range of the batch afterwards (the replay runs those on its pool).
// *end = the bytes the batch uses.
long nsd::reader::scan_batch(nsd_pcap *p, size_t cap, nsd_desc_t *desc, uint64_t *src, uint32_t max_n, size_t *end)
{
	size_t off = 0;
	uint32_t n = 0;
	const uint32_t hs = p->hdrsize;
	*end = 0;
	if (p->eof)
		return 0;
	// (a record read past the index by read_one)
	while (p->ix_i < p->ix_off.size() && p->ix_off[p->ix_i] < p->pos)
		p->ix_i++;
	// (locals: the stores to desc / src could alias p's fields)
	const uint64_t *const ixo = p->ix_off.data();
	const uint32_t *const ixc = p->ix_cap.data();
	const size_t ixn = p->ix_off.size();
	size_t i = p->ix_i;
	long rc = 0;
	while (n < max_n) {
		if (i == ixn) {
			if (p->ix_end)
				p->eof = true;
			break;   // (the caller builds the next window)
		}
		const uint32_t caplen = ixc[i];
		if (caplen > NSD_MAX_CAPLEN) {
			if (n == 0)
				rc = NSD_ERR_CAPLEN;
			break;
		}
		const size_t at = (off + 15) & ~(size_t)15;
		if (at + caplen + NSD_FRAME_PAD > cap) {
			if (n == 0)
				rc = NSD_ERR_ARG;
			break;
		}
		src[n] = ixo[i];
		desc[n] = NSD_DESC(at, caplen);
		i++;
		off = at + caplen;
		n++;
	}
	if (n) {
		p->pos = ixo[i - 1] + hs + ixc[i - 1];
		p->ix_i = i;
	}
	*end = off;
	return rc ? rc : n;
}

// the index window under p->pos is used up (and the walk goes on)
bool nsd::reader::ix_need(const nsd_pcap *p)
{
	size_t i = p->ix_i;
	while (i < p->ix_off.size() && p->ix_off[i] < p->pos)
		i++;
	return i == p->ix_off.size() && !p->ix_end && !p->eof;
}

void nsd::reader::fill_range(const nsd_pcap *p, uint8_t *frames, const nsd_desc_t *desc, const uint64_t *src,
			     uint32_t lo, uint32_t hi, nsd_sll_t *sll, nsd_frame_hdr_t *fh, uint8_t *rhdr)
{
	const uint32_t hs = p->hdrsize;
	for (uint32_t k = lo; k < hi; k++) {
		const uint8_t *h = p->map + src[k];
		memcpy(frames + NSD_DESC_OFF(desc[k]), h + hs, NSD_DESC_CAPLEN(desc[k]));
		if (rhdr)
			memcpy(rhdr + 32 * (size_t)k, h, hs);
		record_meta(p, h, sll + k, fh + k);
	}
}

// ---- a mapped file's record index, built in parallel ----------------------
// The record walk (each header's caplen gives the next header) is one
// dependent load per record: walked by one thread it bounds the replay's
// reader (a 64-byte frame every 80 bytes touches every line of the file).
// A window of the file is cut into chunks; chunk 0 is walked from the exact
// record start, every later chunk from a guess (the first offset from which
// several headers in a row look like records); the exact walk then runs
// through the chunks' results: the exact offset X where it enters chunk c is
// looked up among the offsets chunk c visited, and from there chunk c's walk
// IS the exact walk (a walk is determined by its start).  A chunk whose walk
// never met X (a wrong guess that did not fall into step) is walked again
// from X.  The end rule is read_batch's: a header past the file end, caplen 0
// or > the 1 MiB replay buffer, or a body past the file end ends the walk.
// (IxChunk, one chunk's walk: nsd_pcap_reader.h)

// caplen of the header at pos, or 0 when the end rule stops there
static uint32_t rec_caplen(const nsd_pcap *p, size_t pos)
{
	const uint32_t hs = p->hdrsize;
	if (p->len - pos < hs)
		return 0;
	uint32_t cl;
	memcpy(&cl, p->map + pos + 8, 4);
	if (p->swapped)
		cl = bswap32(cl);
	const uint32_t caplen = cl - p->ll_extra;
	if (caplen == 0 || caplen > REPLAY_BUF || p->len - pos - hs < caplen)
		return 0;
	return caplen;
}

// the walk from pos while pos < stop_at, appended to c
static void ix_walk(const nsd_pcap *p, size_t pos, size_t stop_at, IxChunk &c)
{
	const uint32_t hs = p->hdrsize;
	c.ended = false;
	while (pos < stop_at) {
		if (p->len - pos > 4096 + 64)
			__builtin_prefetch(p->map + pos + 4096);
		const uint32_t caplen = rec_caplen(p, pos);
		if (!caplen) {
			c.ended = true;
			break;
		}
		c.off.push_back(pos);
		c.cap.push_back(caplen);
		pos += hs + caplen;
	}
	c.next = pos;
}

// a record start for a walk from inside [lo, hi): the first offset whose next
// 8 headers pass the end rule with a plausible fraction-of-second field (or
// reach the file end exactly); hi when there is none
static size_t ix_guess(const nsd_pcap *p, size_t lo, size_t hi)
{
	const uint32_t hs = p->hdrsize;
	const uint32_t frac_max = p->nsec ? 1000000000u : 1000000u;
	for (size_t o = lo; o < hi; o++) {
		size_t q = o;
		int k = 0;
		for (; k < 8; k++) {
			if (q == p->len)
				break;
			const uint32_t caplen = rec_caplen(p, q);
			if (!caplen)
				break;
			uint32_t frac;
			memcpy(&frac, p->map + q + 4, 4);
			if ((p->swapped ? bswap32(frac) : frac) >= frac_max)
				break;
			q += hs + caplen;
		}
		if (k == 8 || (k > 0 && q == p->len))
			return o;
	}
	return hi;
}

// chunk c of the window [b[0], b[nc]): walked from its guess to b[c + 1]
void nsd::reader::ix_chunk(const nsd_pcap *p, const std::vector<size_t> &b, int c, IxChunk &out)
{
	out.off.clear();
	out.cap.clear();
	const size_t from = c == 0 ? b[0] : ix_guess(p, b[c], b[c + 1]);
	out.next = from;
	out.ended = false;
	if (from < b[c + 1])
		ix_walk(p, from, b[c + 1], out);
}

// the window's chunk bounds from the exact record start `start`
std::vector<size_t> nsd::reader::ix_bounds(const nsd_pcap *p, size_t start, size_t window, int nc)
{
	const size_t end = p->len - start < window ? p->len : start + window;
	std::vector<size_t> b(nc + 1);
	for (int c = 0; c <= nc; c++)
		b[c] = start + (end - start) * (size_t)c / (size_t)nc;
	b[nc] = end;
	return b;
}

// the exact walk through the chunks' results into p's index
void nsd::reader::ix_splice(nsd_pcap *p, const std::vector<size_t> &b, std::vector<IxChunk> &ch)
{
	const int nc = (int)ch.size();
	p->ix_off.clear();
	p->ix_cap.clear();
	p->ix_i = 0;
	p->ix_end = false;
	size_t x = b[0];
	for (int c = 0; c < nc; c++) {
		if (x >= b[c + 1])
			continue;   // a record across the whole chunk
		IxChunk &k = ch[c];
		const auto it = std::lower_bound(k.off.begin(), k.off.end(), (uint64_t)x);
		if (!(it != k.off.end() && *it == x) && !(k.ended && k.next == x)) {
			// the guess never fell into step: walk the chunk again from x
			k.off.clear();
			k.cap.clear();
			ix_walk(p, x, b[c + 1], k);
			p->ix_off.insert(p->ix_off.end(), k.off.begin(), k.off.end());
			p->ix_cap.insert(p->ix_cap.end(), k.cap.begin(), k.cap.end());
		} else {
			const size_t i = (size_t)(it - k.off.begin());
			p->ix_off.insert(p->ix_off.end(), k.off.begin() + (long)i, k.off.end());
			p->ix_cap.insert(p->ix_cap.end(), k.cap.begin() + (long)i, k.cap.end());
		}
		x = k.next;
		if (k.ended) {
			p->ix_end = true;
			return;
		}
	}
	// the window reached the file end: the walk ends there
	if (b[nc] == p->len && x >= p->len)
		p->ix_end = true;
}

// the index window (bytes of file per build; NSD_PCAP_IX_WINDOW overrides,
// for tests)
size_t nsd::reader::ix_window()
{
	const char *e = getenv("NSD_PCAP_IX_WINDOW");
	const long long v = e ? atoll(e) : 0;
	return v > 0 ? (size_t)v : (size_t)16 << 20;
}

// The record index of a mapped file (the replay reader's, windows of
// `window` bytes, 0 = the replay's, cut into `chunks` walked from guesses and
// spliced): the first max_n records' header offsets and caplens into off /
// caplen.  Returns the records the walk finds (read_batch's end rule), or
// NSD_ERR_ARG (not a pcap file, or not a regular file).
extern "C" long nsd_pcap_index(const char *path, uint64_t window, int chunks, uint64_t *off, uint32_t *caplen,
			       size_t max_n)
{
	nsd_pcap *p = nsd_pcap_open(path);
	if (!p)
		return NSD_ERR_ARG;
	if (!p->map || (max_n && (!off || !caplen))) {
		nsd_pcap_close(p);
		return NSD_ERR_ARG;
	}
	size_t n = 0;
	const int nc = chunks < 1 ? 1 : chunks;
	std::vector<IxChunk> ch(nc);
	while (ix_need(p)) {
		const std::vector<size_t> b = ix_bounds(p, p->pos, window ? (size_t)window : ix_window(), nc);
		// (chunks run last to first: the splice does not depend on the order)
		for (int c = nc - 1; c >= 0; c--)
			ix_chunk(p, b, c, ch[c]);
		ix_splice(p, b, ch);
		for (size_t i = 0; i < p->ix_off.size(); i++, n++)
			if (n < max_n) {
				off[n] = p->ix_off[i];
				caplen[n] = p->ix_cap[i];
			}
		if (!p->ix_off.empty())
			p->pos = p->ix_off.back() + p->hdrsize + p->ix_cap.back();
		p->ix_i = p->ix_off.size();
	}
	nsd_pcap_close(p);
	return (long)n;
}

// The next record whatever its length (<= the 1 MiB replay buffer), for the
// records a batch cannot carry: its bytes into `frame`, its header as stored
// into rhdr (may be NULL), its sockaddr_ll / frame header fields into *sll /
// *fh (record_meta).  Returns caplen, 0 at the end of the replay.
long nsd::reader::read_one(nsd_pcap *p, std::vector<uint8_t> &frame, nsd_sll_t *sll, nsd_frame_hdr_t *fh,
			   uint8_t *rhdr)
{
	if (p->eof || !p->fill(p->hdrsize)) {
		p->eof = true;
		return 0;
	}
	const uint8_t *h = p->data() + p->pos;
	uint32_t cl;
	memcpy(&cl, h + 8, 4);
	if (p->swapped)
		cl = bswap32(cl);
	const uint32_t caplen = cl - p->ll_extra;
	if (caplen == 0 || caplen > REPLAY_BUF || !p->fill((size_t)p->hdrsize + caplen)) {
		p->eof = true;
		return 0;
	}
	h = p->data() + p->pos;
	frame.assign(h + p->hdrsize, h + p->hdrsize + caplen);
	frame.resize((size_t)caplen + NSD_FRAME_PAD, 0);
	if (rhdr)
		memcpy(rhdr, h, p->hdrsize);
	record_meta(p, h, sll, fh);
	p->pos += p->hdrsize + caplen;
	return caplen;
}

// ---- TPACKET_V3 ring front end (walk_t3_block, netsniff-ng.c:990-1039) ------
// A retired RX ring block (struct block_desc, netsniff-ng.c:1061-1066 =
// tpacket_block_desc: version, offset_to_priv, tpacket_hdr_v1 {block_status,
// num_pkts, offset_to_first_pkt, blk_len, seq_num, ts_first, ts_last}) is
// turned into descriptors that point into the block itself, so the block
// is the batch's frame buffer (zero copy on the host; nsd_pipe_submit(block,
// block_len, desc, n, ...)).  Per frame: tpacket3_hdr {tp_next_offset,
// tp_sec, tp_nsec, tp_snaplen, tp_len, tp_status, tp_mac, tp_net, ...} with the
// sockaddr_ll at TPACKET_ALIGN(sizeof(tpacket3_hdr)) = 48 after it; the packet
// is at hdr + tp_mac, tp_snaplen bytes.  skip_packet (netsniff-ng.c:425-442):
// with packet_type >= 0 only frames of that sll_pkttype are kept; otherwise
// frames on the loopback ifindex `lo_ifindex` with PACKET_OUTGOING (4) are
// dropped.  Returns the frames described, or NSD_ERR_ARG for a block whose
// headers point outside it (or a frame above NSD_MAX_CAPLEN).
extern "C" long nsd_t3_block_desc(const uint8_t *block, size_t block_len, int packet_type,
				  int lo_ifindex, nsd_desc_t *desc, uint32_t max_n)
{
	return nsd_t3_block_desc_sll(block, block_len, packet_type, lo_ifindex, desc, nullptr, max_n);
}

// same, also copying each kept frame's sockaddr_ll (hdr + 48, the `sll`
// walk_t3_block hands to dissector_entry_point, netsniff-ng.c:1011-1025)
// into sll[k] (may be NULL): the per-packet input of the SLL heads
extern "C" long nsd_t3_block_desc_sll(const uint8_t *block, size_t block_len, int packet_type,
				      int lo_ifindex, nsd_desc_t *desc, nsd_sll_t *sll, uint32_t max_n)
{
	return nsd_t3_block_desc_fh(block, block_len, packet_type, lo_ifindex, desc, sll, nullptr, max_n);
}

// same, also the frame header fields walk_t3_block's __show_frame_hdr reads
// from each kept frame's tpacket3_hdr (netsniff-ng.c:1021; v3 true):
// tp_sec +4, tp_nsec +8, tp_len +16, tp_status +20, hv1.tp_vlan_tci +32,
// hv1.tp_vlan_tpid +36
extern "C" long nsd_t3_block_desc_fh(const uint8_t *block, size_t block_len, int packet_type, int lo_ifindex,
				     nsd_desc_t *desc, nsd_sll_t *sll, nsd_frame_hdr_t *fh, uint32_t max_n)
{
	if (!block || !desc || block_len < 48)
		return NSD_ERR_ARG;
	uint32_t num_pkts, first;
	memcpy(&num_pkts, block + 12, 4);
	memcpy(&first, block + 16, 4);
	size_t h = first;
	uint32_t n = 0;
	for (uint32_t i = 0; i < num_pkts; i++) {
		if (h + 48 + 20 > block_len)
			return NSD_ERR_ARG;
		uint32_t next, snaplen;
		uint16_t mac;
		int32_t ifindex;
		memcpy(&next, block + h, 4);
		memcpy(&snaplen, block + h + 12, 4);
		memcpy(&mac, block + h + 24, 2);
		memcpy(&ifindex, block + h + 48 + 4, 4);
		const uint8_t pkttype = block[h + 48 + 10];
		const bool skip = packet_type >= 0 ? pkttype != (uint8_t)packet_type
						   : (ifindex == lo_ifindex && pkttype == 4);
		if (!skip) {
			if (h + mac + (size_t)snaplen > block_len || snaplen > NSD_MAX_CAPLEN || n >= max_n)
				return NSD_ERR_ARG;
			if (sll)
				memcpy(&sll[n], block + h + 48, sizeof(nsd_sll_t));
			if (fh) {
				nsd_frame_hdr_t &f = fh[n];
				memset(&f, 0, sizeof(f));
				memcpy(&f.sec, block + h + 4, 4);
				memcpy(&f.nsec, block + h + 8, 4);
				memcpy(&f.len, block + h + 16, 4);
				memcpy(&f.status, block + h + 20, 4);
				memcpy(&f.vlan_tci, block + h + 32, 4);
				memcpy(&f.vlan_tpid, block + h + 36, 2);
				f.v3 = 1;
			}
			desc[n++] = NSD_DESC(h + mac, snaplen);
		}
		if (i + 1 < num_pkts) {
			if (next == 0)
				return NSD_ERR_ARG;
			h += next;
		}
	}
	return n;
}
