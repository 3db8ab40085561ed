// nsd_flow_conv.h - conversations and top-k from the flow table: device code
// of nsd_flow.hip's translation unit, after nsd_flow_table.h.
//
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
#ifndef NSD_FLOW_CONV_H
#define NSD_FLOW_CONV_H

#include "nsd_flow_table.h"

namespace nsdflow {

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
		const uint64_t pos = wave_cursor(&w.h->ncand, m, lane);
		if (own) {
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
// and k - rem .. k - 1, each through a wave-aggregated cursor.  TS: nsd_convt
// rows, the smaller t_first and the larger t_last of the row's slot and `rev`.
template <bool TS>
__global__ __launch_bounds__(BLOCK) void conv_gather(Tab t, ConvWs w, uint32_t k, uint64_t *out, uint32_t *count)
{
	constexpr uint64_t ROW = TS ? 13 : 11;
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
	const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
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
		uint64_t pos = UINT64_MAX;
		if (ma) {   // (wave-uniform, as mt)
			const uint64_t p = wave_cursor(&h->n_above, ma, lane);
			if (above)
				pos = p;
		}
		if (mt) {
			const uint64_t j = wave_cursor(&h->n_tied, mt, lane);
			if (tied && j < rem)
				pos = base + j;
		}
		if (pos >= k)
			continue;
		const uint32_t s = w.slot[i], r = w.rev[i];
		if (s >= t.slots || (r != NOSLOT && r >= t.slots))
			continue;
		// (the key word by word from the table, not load_key: five words held
		// beside both directions' counters cost this kernel six to ten registers)
		const uint64_t *kp = t.key + 5ull * s;
		const Cnt c = t.cnt[s];
		Cnt e = empty_cnt();
		if (r != NOSLOT)
			e = t.cnt[r];
		uint64_t *o = out + ROW * pos;
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
		if constexpr (TS) {
			uint64_t tf = t.tm[2ull * s], tl = t.tm[2ull * s + 1];
			if (r != NOSLOT) {
				const uint64_t rf = t.tm[2ull * r], rl = t.tm[2ull * r + 1];
				tf = rf < tf ? rf : tf;
				tl = rl > tl ? rl : tl;
			}
			o[11] = tf;
			o[12] = tl;
		}
	}
}

} // namespace nsdflow

#endif /* NSD_FLOW_CONV_H */
