// nsd_flow_cpu.cpp - the flow table's aggregation on the host CPU: flows from
// records (nsd_flow_cpu), conversations from flow rows (nsd_conv_cpu) and the
// expiry rules over flow rows (nsd_flow_expire_cpu), each in its plain and its
// _ts form.  The key function is the kernels' (nsd_flow.h); nothing here
// touches a GPU.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "nsd_flow.h"
#include "nsd_internal.h"

using namespace nsdflow;

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
