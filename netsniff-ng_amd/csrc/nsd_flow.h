// nsd_flow.h - the flow key of one dissected packet, shared by the device
// kernels (nsd_flow.hip) and the host aggregation (nsd_flow_cpu.cpp).
//
// The reference shows per-flow packet and byte counters in flowtop
// (flowtop.c: struct flow_entry's pkts_src / bytes_src, taken from
// conntrack's CTA_COUNTERS); here they are taken from a dissected batch: the
// record (and its ext-pool entry) names every layer and where it starts, so
// the key is a handful of byte loads at known offsets.
//
// Rules (include/netsniff_dissect.h "flow table"):
//   L3  = the first layer whose ops id is NSD_OPS_IPV4 / NSD_OPS_IPV6 (the
//         outermost; none: the packet is not keyed, NSD_FLOW_ST_NOIP);
//   L4  = the last layer of the chain; ports from TCP / UDP / DCCP only, and
//         not from a later IPv4 fragment (the reference still dispatches such
//         a packet to tcp, but the bytes there are no TCP header);
//   bytes at offsets >= caplen read as zero (the parity domain's rule,
//   nsd_walk.h / nsd_cpu.hip), caplen capped at NSD_MAX_CAPLEN for the key.
#ifndef NSD_FLOW_H
#define NSD_FLOW_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/netsniff_dissect.h"

#define NSD_FHD __host__ __device__ __forceinline__

namespace nsdflow {

// bytes 0..39 of nsd_flow as five little-endian u64 words: src, dst, then
// sport | dport << 16 | l3 << 32 | l4 << 40 (tcp_flags / rsvd bytes zero)
struct Key {
	uint64_t w[5];
};

enum { K_KEYED = 0, K_NOIP = 1, K_SKIPPED = 2 };

// bytes of one frame, zero at offsets >= caplen
struct Src {
	const uint8_t *p;
	uint32_t caplen;

	NSD_FHD uint32_t b(uint32_t o) const { return o < caplen ? p[o] : 0u; }
	NSD_FHD uint32_t be16(uint32_t o) const { return b(o) << 8 | b(o + 1); }
	// 8 bytes at o as a little-endian word (memory order)
	NSD_FHD uint64_t le64(uint32_t o) const
	{
		if (o + 8 <= caplen) {
			uint64_t v;
			memcpy(&v, p + o, 8);
			return v;
		}
		uint64_t v = 0;
		for (uint32_t k = 0; k < 8; k++)
			v |= (uint64_t)b(o + k) << (8 * k);
		return v;
	}
	NSD_FHD uint64_t le32(uint32_t o) const
	{
		if (o + 4 <= caplen) {
			uint32_t v;
			memcpy(&v, p + o, 4);
			return v;
		}
		return b(o) | b(o + 1) << 8 | b(o + 2) << 16 | b(o + 3) << 24;
	}
};

// The key of one packet from its record, the ext pool its slot refers to
// (ext_words = the pool's size; entries that leave it are skipped) and its
// frame.  Returns K_KEYED (key / tflags set), K_NOIP or K_SKIPPED.
NSD_FHD int flow_key(const nsd_rec &r, const uint32_t *ext, uint32_t ext_words, const uint8_t *frame,
		     uint32_t caplen, Key &key, uint32_t &tflags)
{
	tflags = 0;
	if (r.nflags & NSD_F_OVERFLOW)
		return K_SKIPPED;
	const Src s{ frame, caplen < NSD_MAX_CAPLEN ? caplen : NSD_MAX_CAPLEN };
	uint32_t nl = r.nflags & 7u;
	uint32_t l3 = 0, l3off = 0, l4 = 0, l4off = 0;
	// off2[0..4] in one word (no indexed byte array: that would live in scratch)
	const uint64_t o2 = (uint64_t)r.off2[0] | (uint64_t)r.off2[1] << 8 | (uint64_t)r.off2[2] << 16 |
			    (uint64_t)r.off2[3] << 24 | (uint64_t)r.off2[4] << 32;
	if (nl == NSD_N_EXT) {
		const uint32_t slot = (uint32_t)o2;
		if (!ext || (uint64_t)slot + NSD_EXT_HDR_WORDS > ext_words)
			return K_SKIPPED;
		nl = NSD_EXT_NLAYERS(ext, slot);
		if (nl > NSD_EXT_MAX_LAYERS)
			nl = NSD_EXT_MAX_LAYERS;
		if ((uint64_t)slot + NSD_EXT_HDR_WORDS + nl > ext_words)
			return K_SKIPPED;
		for (uint32_t k = 0; k < nl; k++) {
			const uint32_t id = NSD_EXT_ID(ext, slot, k);
			if (id == NSD_OPS_IPV4 || id == NSD_OPS_IPV6) {
				l3 = id;
				l3off = NSD_EXT_OFF(ext, slot, k);
				break;
			}
		}
		if (nl) {
			l4 = NSD_EXT_ID(ext, slot, nl - 1);
			l4off = NSD_EXT_OFF(ext, slot, nl - 1);
		}
	} else {
		for (uint32_t k = 0; k < nl; k++) {
			const uint32_t id = (r.chain >> (5u * k)) & 31u;
			if (id == NSD_OPS_IPV4 || id == NSD_OPS_IPV6) {
				l3 = id;
				l3off = k ? 2u * (uint32_t)((o2 >> (8u * (k - 1))) & 255u) : 0u;
				break;
			}
		}
		if (nl) {
			l4 = (r.chain >> (5u * (nl - 1))) & 31u;
			l4off = nl > 1 ? 2u * (uint32_t)((o2 >> (8u * (nl - 2))) & 255u) : 0u;
		}
	}
	if (!l3)
		return K_NOIP;
	bool later_frag = false;
	if (l3 == NSD_OPS_IPV4) {
		key.w[0] = s.le32(l3off + 12);
		key.w[1] = 0;
		key.w[2] = s.le32(l3off + 16);
		key.w[3] = 0;
		later_frag = (s.be16(l3off + 6) & 0x1fffu) != 0;
	} else {
		key.w[0] = s.le64(l3off + 8);
		key.w[1] = s.le64(l3off + 16);
		key.w[2] = s.le64(l3off + 24);
		key.w[3] = s.le64(l3off + 32);
	}
	uint32_t sport = 0, dport = 0;
	if (!later_frag && (l4 == NSD_OPS_TCP || l4 == NSD_OPS_UDP || l4 == NSD_OPS_DCCP)) {
		sport = s.be16(l4off);
		dport = s.be16(l4off + 2);
		if (l4 == NSD_OPS_TCP)
			tflags = s.b(l4off + 13);
	}
	key.w[4] = (uint64_t)sport | (uint64_t)dport << 16 | (uint64_t)l3 << 32 | (uint64_t)l4 << 40;
	return K_KEYED;
}

NSD_FHD bool key_eq(const Key &a, const Key &b)
{
	return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3]) | (a.w[4] ^ b.w[4])) == 0;
}

// 64-bit mix of the five words (the multiply / xor-shift finaliser of
// splitmix64 per word); the table index is its low bits
NSD_FHD uint64_t key_hash(const Key &k)
{
	uint64_t h = 0x9E3779B97F4A7C15ull;
	for (int i = 0; i < 5; i++) {
		h ^= k.w[i];
		h *= 0xBF58476D1CE4E5B9ull;
		h ^= h >> 29;
	}
	h *= 0x94D049BB133111EBull;
	return h ^ (h >> 32);
}

} // namespace nsdflow

#endif /* NSD_FLOW_H */
