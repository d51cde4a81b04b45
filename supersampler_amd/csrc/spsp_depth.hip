// Depth on the GPU: how many records of a read set hold each key of an index, and per reference how many of its keys were seen and
// what their typical count is (not in the reference, whose end product is the two n x n matrices).
//
// The index is the classification's (spsp_classify.hip): references 0 .. R-1 with key sets K_j, U their union, D = |U|, h(x) the
// references that hold x; the prevalence table names a key's claimer entry, key_no[claimer] the key's number in 0 .. D-1, and
// key_start[number + 1] - key_start[number] = h.  Records r have distinct key sets Q_r.
//   c(x) = #{r : x in Q_r}          found at min_count: c(x) >= min_count
// Per reference j over F_j = {x in K_j : found}: keys, found, sum, max and the lower median of c; the same five over the keys with
// h == 1.  Integers only; the answer is a function of the multiset of record keys (integer adds commute).
//
// begin (once per index):
//   k_dp_number  a lane per index entry: the probe of the table (pv_find) for the entry's own key -> kn[at] = the key's number,
//                uniq[at] = (h == 1).  An entry that is not its key's claimer does not know its key's number otherwise.  The
//                counters, one 32-bit word per distinct key, are cleared.
// add (any number of times, no host wait):
//   k_dp_add     a lane per record key: pv_find, and on a hit one no-return atomic add of 1 to count[number]; the wave's hits are
//                summed and added once to the 64-bit hit-keys word.  Bound: one random 8-byte slot read and one 20- or 28-byte key
//                read per record key, one 4-byte atomic at L2 per hit.
// read (one host wait; the counters stay):
//   k_dp_entry   a lane per index entry: c_e[at] = count[kn[at]], coalesced but for the count; the lanes below D also count the
//                keys found (one add per wave).  Bound: 12 bytes per entry.
//   k_dp_reduce  a workgroup per reference, references strided over the grid.  It streams c_e and uniq coalesced into two LDS
//                histograms of kDpBins bins (all keys | unique keys; the last bin holds every count at or above kDpBins - 1) while
//                found, sum and max are kept in registers and reduced over the workgroup; the median is found by a scan of the
//                histogram, and where its rank lands in the last bin, by a radix select over the values at or above kDpBins - 1:
//                four passes of 256 bins over the same stream.  Bound: 5 bytes per entry and pass.
//   k_dp_segment, k_dp_merge   a reference of more than kDpLongKeys entries is left out of k_dp_reduce: a workgroup per segment of
//                kDpSegKeys entries adds its histograms and sums to the reference's words in device memory, and one workgroup per
//                such reference finishes the row from them (measured: one workgroup on 4 x 10^6 entries was 93 % of a read).
// No workgroup waits for another.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kDpWaves = kDpThreads / 64;
constexpr uint32_t kDpPerLane = kDpBins / kDpThreads;     // bins one lane scans
static_assert(kDpBins % kDpThreads == 0 && kDpBins >= 2, "a lane scans a whole number of bins");
enum { kDpwHit = 0, kDpwFound = 1, kDpWords = 2 };         // the 64-bit total words: hit keys since begin, index keys found at the last read

template <bool HAS_HI>
__global__ __launch_bounds__(kDpThreads) void k_dp_number(SortedKeys K, uint64_t first, uint32_t n_index, const unsigned long long* __restrict__ tbl,
                                                          uint32_t log2cap, const uint32_t* __restrict__ key_no, const uint32_t* __restrict__ key_start,
                                                          uint32_t D, uint32_t* __restrict__ kn, uint8_t* __restrict__ uniq) {
    const uint64_t i = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x;
    if (i >= n_index) return;
    const uint64_t e = first + i;
    const uint64_t at = pv_find<HAS_HI>(K, first, n_index, tbl, log2cap, K.mn[e], HAS_HI ? K.hi[e] : 0ull, K.lo[e]);
    uint32_t number = 0xffffffffu, u = 0;
    if (at != ~0ull) {                                     // (always: the table was filled from these entries)
        number = key_no[at];
        if (number < D) u = key_start[number + 1u] - key_start[number] == 1u;
        else number = 0xffffffffu;
    }
    kn[i] = number;
    uniq[i] = (uint8_t)u;
}

// Q: the record keys, entries [q0, q0 + n_keys); K, tbl, key_no: the index (first: its first entry, n_index: its entries, D: its distinct keys)
template <bool HAS_HI>
__global__ __launch_bounds__(kDpThreads) void k_dp_add(SortedKeys Q, uint64_t q0, uint32_t n_keys, SortedKeys K, uint64_t first, uint32_t n_index,
                                                       const unsigned long long* __restrict__ tbl, uint32_t log2cap, const uint32_t* __restrict__ key_no,
                                                       uint32_t D, uint32_t* __restrict__ count, unsigned long long* __restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x;
    uint32_t hit = 0;
    if (i < n_keys) {
        const uint64_t e = q0 + i;
        const uint64_t at = pv_find<HAS_HI>(K, first, n_index, tbl, log2cap, Q.mn[e], HAS_HI ? Q.hi[e] : 0ull, Q.lo[e]);
        if (at != ~0ull) {
            const uint32_t number = key_no[at];
            if (number < D) { atomicAdd(&count[number], 1u); hit = 1; }   // (the value is not used: an add without a return)
        }
    }
    const uint32_t hits = (uint32_t)__popcll(__ballot(hit != 0u));
    if ((threadIdx.x & 63u) == 0u && hits) atomicAdd(&words[kDpwHit], (unsigned long long)hits);
}

__global__ __launch_bounds__(kDpThreads) void k_dp_entry(const uint32_t* __restrict__ kn, uint32_t n_index, const uint32_t* __restrict__ count, uint32_t D,
                                                         uint32_t min_count, uint32_t* __restrict__ c_e, unsigned long long* __restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x;
    if (i < n_index) {
        const uint32_t number = kn[i];
        c_e[i] = number < D ? count[number] : 0u;
    }
    // the keys found: the lanes below D (D <= n_index: the grid covers them)
    const uint32_t found = (uint32_t)__popcll(__ballot(i < D && count[i < D ? i : 0] >= min_count));
    if ((threadIdx.x & 63u) == 0u && found) atomicAdd(&words[kDpwFound], (unsigned long long)found);
}

// sums over the workgroup: every lane gets the total.  s: kDpWaves words nobody else uses between the two barriers inside
__device__ __forceinline__ unsigned long long dp_block_sum(unsigned long long v, unsigned long long* s) {
    v = wave_sum(v);
    __syncthreads();                                       // (the last use of s is over)
    if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDpWaves; ++w) t += s[w];
    return t;
}
__device__ __forceinline__ uint32_t dp_block_max(uint32_t v, unsigned long long* s) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDpWaves; ++w) t = max(t, (uint32_t)s[w]);
    return t;
}
// the exclusive prefix of v over the workgroup's lanes in lane order
__device__ __forceinline__ uint32_t dp_block_prefix(uint32_t v, unsigned long long* s) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t incl = wave_prefix_incl(v, lane);
    __syncthreads();
    if (lane == 63u) s[wid] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < kDpWaves; ++w) if (w < wid) before += (uint32_t)s[w];
    return before + incl - v;
}

// the value of rank `rank` (from 0, ascending) among the found counts at or above kDpBins - 1 of entries [a, z), of the unique keys
// alone where only_unique: four passes over the stream, most significant byte first.  s_bin: 256 words; s_pick: 2 words.  Uniform
__device__ uint32_t dp_select(const uint32_t* __restrict__ c_e, const uint8_t* __restrict__ uniq, uint64_t a, uint64_t z, bool only_unique, uint32_t floor_c,
                              uint32_t rank, uint32_t* s_bin, uint32_t* s_pick, unsigned long long* s_red) {
    uint32_t prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();
        s_bin[threadIdx.x] = 0u;                           // (kDpThreads == 256 bins)
        __syncthreads();
        for (uint64_t i = a + threadIdx.x; i < z; i += kDpThreads) {
            const uint32_t c = c_e[i];
            if (c < floor_c || (only_unique && !uniq[i])) continue;
            if (shift < 24 && (c >> (shift + 8)) != prefix) continue;
            atomicAdd(&s_bin[(c >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t mine = s_bin[threadIdx.x], before = dp_block_prefix(mine, s_red);
        if (rank >= before && rank < before + mine) { s_pick[0] = threadIdx.x; s_pick[1] = rank - before; }   // (exactly one lane: the rank is below the total)
        __syncthreads();
        prefix = (prefix << 8) | s_pick[0];
        rank = s_pick[1];
    }
    return prefix;
}

// the bin that holds rank `rank` of a histogram of kDpBins bins, and the rank inside it -> s_pick[0], s_pick[1].  Uniform
__device__ __forceinline__ void dp_hist_rank(const uint32_t* s_hist, uint32_t rank, uint32_t* s_pick, unsigned long long* s_red) {
    uint32_t part = 0;
#pragma unroll
    for (uint32_t b = 0; b < kDpPerLane; ++b) part += s_hist[threadIdx.x * kDpPerLane + b];
    uint32_t before = dp_block_prefix(part, s_red);
    if (rank >= before && rank < before + part) {          // (exactly one lane)
        for (uint32_t b = 0; b < kDpPerLane; ++b) {
            const uint32_t n = s_hist[threadIdx.x * kDpPerLane + b];
            if (rank < before + n) { s_pick[0] = threadIdx.x * kDpPerLane + b; s_pick[1] = rank - before; break; }
            before += n;
        }
    }
    __syncthreads();
}

static_assert(kDpThreads == 256, "dp_select's bins are one per lane");

// what one pass over entries [a, z) leaves beside the two histograms: the sums over the workgroup, in every lane
struct DpPart { unsigned long long sum, usum; uint32_t found, ufound, ukeys, mx, umx; };

// s_hist (cleared by the caller, behind a barrier) += the found counts of entries [a, z) by bin.  Uniform; a barrier behind it
__device__ __forceinline__ DpPart dp_stream(const uint32_t* __restrict__ c_e, const uint8_t* __restrict__ uniq, uint64_t a, uint64_t z, uint32_t min_count,
                                            uint32_t (*s_hist)[kDpBins], unsigned long long* s_red) {
    unsigned long long sum = 0, usum = 0;
    uint32_t found = 0, ufound = 0, mx = 0, umx = 0, ukeys = 0;
    for (uint64_t i = a + threadIdx.x; i < z; i += kDpThreads) {
        const uint32_t c = c_e[i], u = uniq[i];
        ukeys += u;
        if (c < min_count) continue;
        const uint32_t bin = min(c, kDpBins - 1u);
        ++found; sum += c; mx = max(mx, c);
        atomicAdd(&s_hist[0][bin], 1u);
        if (u) { ++ufound; usum += c; umx = max(umx, c); atomicAdd(&s_hist[1][bin], 1u); }
    }
    __syncthreads();
    DpPart p;
    p.found = (uint32_t)dp_block_sum(found, s_red);
    p.ufound = (uint32_t)dp_block_sum(ufound, s_red);
    p.ukeys = (uint32_t)dp_block_sum(ukeys, s_red);
    p.sum = dp_block_sum(sum, s_red);
    p.usum = dp_block_sum(usum, s_red);
    p.mx = dp_block_max(mx, s_red);
    p.umx = dp_block_max(umx, s_red);
    return p;
}

// the row of reference entries [a, z) from its sums and its two histograms in LDS.  Uniform
__device__ __forceinline__ spsp_depth_row dp_finish(const DpPart& p, const uint32_t* __restrict__ c_e, const uint8_t* __restrict__ uniq, uint64_t a, uint64_t z,
                                                    uint32_t min_count, uint32_t (*s_hist)[kDpBins], uint32_t* s_bin, uint32_t* s_pick, unsigned long long* s_red) {
    const uint32_t floor_c = max(min_count, kDpBins - 1u);  // what a found value of the last bin is at least
    spsp_depth_row row;
    row.keys = (uint32_t)(z - a);
    row.found = p.found; row.unique_found = p.ufound; row.unique_keys = p.ukeys;
    row.sum = p.sum; row.unique_sum = p.usum; row.max = p.mx; row.unique_max = p.umx;
    row.median = row.unique_median = 0;
    for (uint32_t which = 0; which < 2u; ++which) {        // (uniform)
        const uint32_t n = which ? row.unique_found : row.found;
        if (n == 0u) continue;
        dp_hist_rank(s_hist[which], (n - 1u) >> 1, s_pick, s_red);
        uint32_t median = s_pick[0];
        const uint32_t inside = s_pick[1];
        if (median == kDpBins - 1u) median = dp_select(c_e, uniq, a, z, which != 0u, floor_c, inside, s_bin, s_pick, s_red);
        if (which) row.unique_median = median; else row.median = median;
        __syncthreads();                                   // (s_pick is read: the next round writes it)
    }
    return row;
}

// off: the references' first entries as the index call uploaded them (absolute; off[0] = the index's first entry).  A reference
// of more than kDpLongKeys entries is left to k_dp_segment and k_dp_merge.  Four workgroups per CU: what the two histograms leave room for
__global__ __launch_bounds__(kDpThreads, 4) void k_dp_reduce(const uint64_t* __restrict__ off, uint32_t n_ref, const uint32_t* __restrict__ c_e,
                                                          const uint8_t* __restrict__ uniq, uint32_t min_count, spsp_depth_row* __restrict__ rows) {
    __shared__ uint32_t s_hist[2][kDpBins];
    __shared__ uint32_t s_bin[256];
    __shared__ uint32_t s_pick[2];
    __shared__ unsigned long long s_red[kDpWaves];
    const uint64_t first = off[0];
    for (uint32_t j = blockIdx.x; j < n_ref; j += gridDim.x) {   // (uniform per workgroup)
        const uint64_t a = off[j] - first, z = off[j + 1] - first;
        if (z - a > kDpLongKeys) continue;
        __syncthreads();                                   // (the last reference's histograms are read)
        for (uint32_t b = threadIdx.x; b < 2u * kDpBins; b += kDpThreads) (&s_hist[0][0])[b] = 0u;
        __syncthreads();
        const DpPart p = dp_stream(c_e, uniq, a, z, min_count, s_hist, s_red);
        const spsp_depth_row row = dp_finish(p, c_e, uniq, a, z, min_count, s_hist, s_bin, s_pick, s_red);
        if (threadIdx.x == 0u) rows[j] = row;
    }
}

// the long references by segments of kDpSegKeys entries, a workgroup per segment: segment b is segment seg_no[b] of long reference
// seg_long[b], which is reference long_ref[.]; its sums go to acc[l][0 .. kDpAccWords) and its bins to hist[l] by atomic adds
// (integer adds: whatever the order, the same words)
enum { kDpaSum = 0, kDpaUsum = 1, kDpaFound = 2, kDpaUfound = 3, kDpaUkeys = 4, kDpaMax = 5, kDpaUmax = 6, kDpAccWords = 8 };
__global__ __launch_bounds__(kDpThreads) void k_dp_segment(const uint64_t* __restrict__ off, const uint32_t* __restrict__ long_ref, const uint32_t* __restrict__ seg_long,
                                                           const uint32_t* __restrict__ seg_no, const uint32_t* __restrict__ c_e, const uint8_t* __restrict__ uniq,
                                                           uint32_t min_count, uint32_t* __restrict__ hist, unsigned long long* __restrict__ acc) {
    __shared__ uint32_t s_hist[2][kDpBins];
    __shared__ unsigned long long s_red[kDpWaves];
    const uint32_t l = seg_long[blockIdx.x], j = long_ref[l];
    const uint64_t first = off[0], end = off[j + 1] - first;
    const uint64_t a = off[j] - first + (uint64_t)seg_no[blockIdx.x] * kDpSegKeys, z = min(end, a + (uint64_t)kDpSegKeys);
    for (uint32_t b = threadIdx.x; b < 2u * kDpBins; b += kDpThreads) (&s_hist[0][0])[b] = 0u;
    __syncthreads();
    const DpPart p = dp_stream(c_e, uniq, min(a, end), z, min_count, s_hist, s_red);
    uint32_t* g = hist + (size_t)l * 2u * kDpBins;
    for (uint32_t b = threadIdx.x; b < 2u * kDpBins; b += kDpThreads) { const uint32_t v = (&s_hist[0][0])[b]; if (v) atomicAdd(g + b, v); }
    if (threadIdx.x == 0u) {
        unsigned long long* w = acc + (size_t)l * kDpAccWords;
        if (p.ukeys) atomicAdd(w + kDpaUkeys, (unsigned long long)p.ukeys);
        if (p.found) {
            atomicAdd(w + kDpaSum, p.sum); atomicAdd(w + kDpaFound, (unsigned long long)p.found); atomicMax(w + kDpaMax, (unsigned long long)p.mx);
        }
        if (p.ufound) {
            atomicAdd(w + kDpaUsum, p.usum); atomicAdd(w + kDpaUfound, (unsigned long long)p.ufound); atomicMax(w + kDpaUmax, (unsigned long long)p.umx);
        }
    }
}

// a workgroup per long reference: the segments' histograms and sums -> its row
__global__ __launch_bounds__(kDpThreads) void k_dp_merge(const uint64_t* __restrict__ off, const uint32_t* __restrict__ long_ref, const uint32_t* __restrict__ c_e,
                                                         const uint8_t* __restrict__ uniq, uint32_t min_count, const uint32_t* __restrict__ hist,
                                                         const unsigned long long* __restrict__ acc, spsp_depth_row* __restrict__ rows) {
    __shared__ uint32_t s_hist[2][kDpBins];
    __shared__ uint32_t s_bin[256];
    __shared__ uint32_t s_pick[2];
    __shared__ unsigned long long s_red[kDpWaves];
    const uint32_t l = blockIdx.x, j = long_ref[l];
    const uint64_t first = off[0], a = off[j] - first, z = off[j + 1] - first;
    const uint32_t* g = hist + (size_t)l * 2u * kDpBins;
    for (uint32_t b = threadIdx.x; b < 2u * kDpBins; b += kDpThreads) (&s_hist[0][0])[b] = g[b];
    const unsigned long long* w = acc + (size_t)l * kDpAccWords;
    DpPart p;
    p.sum = w[kDpaSum]; p.usum = w[kDpaUsum]; p.found = (uint32_t)w[kDpaFound]; p.ufound = (uint32_t)w[kDpaUfound]; p.ukeys = (uint32_t)w[kDpaUkeys];
    p.mx = (uint32_t)w[kDpaMax]; p.umx = (uint32_t)w[kDpaUmax];
    __syncthreads();
    const spsp_depth_row row = dp_finish(p, c_e, uniq, a, z, min_count, s_hist, s_bin, s_pick, s_red);
    if (threadIdx.x == 0u) rows[j] = row;
}

const char* const kNoDepth = "depth: the context holds no counters (spsp_depth_begin_device first; they end with the index they were made for)";

}  // namespace

int depth_begin_impl(spsp_ctx* ctx) {
    int rc;
    spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    if (!X.valid) return refuse_no_index("classification");
    X.depth = false;
    const uint32_t E = X.entries;
    uint32_t D = 0;
    // the references of more than kDpLongKeys entries and their segments: long_ref [n_long] | seg_long [n_seg] | seg_no [n_seg]
    std::vector<uint32_t> long_ref, seg_long, seg_no;
    for (uint32_t j = 0; E && j < X.n_ref; ++j) {
        const uint64_t keys = X.off_host[j + 1] - X.off_host[j];
        if (keys <= kDpLongKeys) continue;
        for (uint64_t sg = 0; sg * kDpSegKeys < keys; ++sg) { seg_long.push_back((uint32_t)long_ref.size()); seg_no.push_back((uint32_t)sg); }
        long_ref.push_back(j);
    }
    ctx->dp_n_long = (uint32_t)long_ref.size(); ctx->dp_n_seg = (uint32_t)seg_long.size();
    if (E) {
        if (ctx->dp_n_long) {
            const size_t nl = long_ref.size(), ns = seg_long.size();
            if ((rc = ctx->dp_long.reserve((nl + 2 * ns) * 4)) || (rc = ctx->dp_hist.reserve(nl * (2 * kDpBins * 4 + kDpAccWords * 8)))) return rc;
            uint32_t* d = ctx->dp_long.as<uint32_t>();
            SPSP_HIP(hipMemcpyAsync(d, long_ref.data(), nl * 4, hipMemcpyHostToDevice, ctx->stream));
            SPSP_HIP(hipMemcpyAsync(d + nl, seg_long.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
            SPSP_HIP(hipMemcpyAsync(d + nl + ns, seg_no.data(), ns * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        SPSP_HIP(hipMemcpyAsync(&D, X.key_no + E, 4, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // begin's wait (the three host arrays above live until here)
        if (D == 0 || D > E) { set_error("depth: the index names %u distinct keys for %u entries (the index arrays changed?)", D, E); return SPSP_ERR_ARG; }
    }
    if ((rc = ctx->dp_count.reserve((size_t)D * 4 + 64)) || (rc = ctx->dp_kn.reserve((size_t)E * 4 + 64)) || (rc = ctx->dp_uniq.reserve((size_t)E + 64)) ||
        (rc = ctx->dp_words.reserve(kDpWords * 8))) return rc;
    SPSP_HIP(hipMemsetAsync(ctx->dp_count.p, 0, (size_t)D * 4 + 64, ctx->stream));
    SPSP_HIP(hipMemsetAsync(ctx->dp_words.p, 0, kDpWords * 8, ctx->stream));
    if (E) {
        const SortedKeys K{X.mn, X.lo, X.hi};
        const unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
        const uint32_t gx = (uint32_t)(((uint64_t)E + kDpThreads - 1) / kDpThreads);
        if (X.has_hi) hipLaunchKernelGGL(k_dp_number<true>, dim3(gx), dim3(kDpThreads), 0, ctx->stream, K, X.first, E, d_tbl, ctx->pv_log2cap, X.key_no, X.key_start, D,
                                         ctx->dp_kn.as<uint32_t>(), ctx->dp_uniq.as<uint8_t>());
        else hipLaunchKernelGGL(k_dp_number<false>, dim3(gx), dim3(kDpThreads), 0, ctx->stream, K, X.first, E, d_tbl, ctx->pv_log2cap, X.key_no, X.key_start, D,
                                ctx->dp_kn.as<uint32_t>(), ctx->dp_uniq.as<uint8_t>());
        SPSP_HIP(hipGetLastError());
    }
    X.distinct = D;
    X.depth = true;
    ctx->dp_record_keys = 0;
    return SPSP_OK;
}

int depth_add_impl(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, uint64_t first, uint64_t n_keys) {
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    if (!X.valid || !X.depth) { set_error("%s", kNoDepth); return SPSP_ERR_ARG; }
    if (int rc = record_keys_check(ctx, "depth", q_mn, q_lo, q_hi, n_keys)) return rc;
    if (n_keys > 0xfffffff0ull) { set_error("too many record keys for one call"); return SPSP_ERR_OVERFLOW; }
    if (ctx->dp_record_keys + n_keys > 0xffffffffull) {
        set_error("depth: more than 4 294 967 295 record keys since spsp_depth_begin_device (a 32-bit counter could wrap)");
        return SPSP_ERR_OVERFLOW;
    }
    ctx->dp_record_keys += n_keys;
    if (n_keys == 0 || X.entries == 0) return SPSP_OK;
    const SortedKeys Q{q_mn, q_lo, q_hi}, K{X.mn, X.lo, X.hi};
    const unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
    const uint32_t gx = (uint32_t)((n_keys + kDpThreads - 1) / kDpThreads);
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (ctx->timing) {                                     // spsp_timing_enable: a pair of events around the launch (spsp_depth_stage_ms reads them)
        if (!ctx->dp_add_spare.empty()) { ev = ctx->dp_add_spare.back(); ctx->dp_add_spare.pop_back(); }
        else { SPSP_HIP(hipEventCreate(&ev.first)); SPSP_HIP(hipEventCreate(&ev.second)); }
        ctx->dp_add_used.push_back(ev);
        SPSP_HIP(hipEventRecord(ev.first, ctx->stream));
    }
    if (X.has_hi) hipLaunchKernelGGL(k_dp_add<true>, dim3(gx), dim3(kDpThreads), 0, ctx->stream, Q, first, (uint32_t)n_keys, K, X.first, X.entries, d_tbl,
                                     ctx->pv_log2cap, X.key_no, X.distinct, ctx->dp_count.as<uint32_t>(), ctx->dp_words.as<unsigned long long>());
    else hipLaunchKernelGGL(k_dp_add<false>, dim3(gx), dim3(kDpThreads), 0, ctx->stream, Q, first, (uint32_t)n_keys, K, X.first, X.entries, d_tbl,
                            ctx->pv_log2cap, X.key_no, X.distinct, ctx->dp_count.as<uint32_t>(), ctx->dp_words.as<unsigned long long>());
    SPSP_HIP(hipGetLastError());
    if (ev.second) SPSP_HIP(hipEventRecord(ev.second, ctx->stream));
    return SPSP_OK;
}

int depth_launch_entry(spsp_ctx* ctx, uint32_t min_count, unsigned long long** d_found) {
    int rc;
    const uint32_t E = ctx->cf_index.entries, D = ctx->cf_index.distinct;
    if ((rc = ctx->dp_entry.reserve((size_t)E * 4 + 64))) return rc;
    unsigned long long* d_words = ctx->dp_words.as<unsigned long long>();
    if (d_found) *d_found = d_words + kDpwFound;
    SPSP_HIP(hipMemsetAsync(d_words + kDpwFound, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_dp_entry, dim3((uint32_t)(((uint64_t)E + kDpThreads - 1) / kDpThreads)), dim3(kDpThreads), 0, ctx->stream,
                       (const uint32_t*)ctx->dp_kn.as<uint32_t>(), E, (const uint32_t*)ctx->dp_count.as<uint32_t>(), D, min_count, ctx->dp_entry.as<uint32_t>(), d_words);
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

int depth_launch_reduce(spsp_ctx* ctx, const uint8_t* d_class, uint32_t min_count, spsp_depth_row* d_rows) {
    const uint32_t R = ctx->cf_index.n_ref;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(R, (uint64_t)std::max(ctx->n_cu, 1) * 4u);
    const uint64_t* d_off = ctx->pv_off.as<uint64_t>();
    const uint32_t* d_c = ctx->dp_entry.as<uint32_t>();
    hipLaunchKernelGGL(k_dp_reduce, dim3(grid), dim3(kDpThreads), 0, ctx->stream, d_off, R, d_c, d_class, min_count, d_rows);
    if (ctx->dp_n_long) {                                  // the long references: their segments, then one merge per reference
        const size_t nl = ctx->dp_n_long, ns = ctx->dp_n_seg;
        const uint32_t *d_long = ctx->dp_long.as<uint32_t>(), *d_seg_long = d_long + nl, *d_seg_no = d_seg_long + ns;
        unsigned long long* d_acc = ctx->dp_hist.as<unsigned long long>();       // (the 64-bit words in front: aligned)
        uint32_t* d_hist = reinterpret_cast<uint32_t*>(d_acc + nl * kDpAccWords);
        SPSP_HIP(hipMemsetAsync(d_acc, 0, nl * (2 * kDpBins * 4 + kDpAccWords * 8), ctx->stream));
        hipLaunchKernelGGL(k_dp_segment, dim3((uint32_t)ns), dim3(kDpThreads), 0, ctx->stream, d_off, d_long, d_seg_long, d_seg_no, d_c, d_class, min_count, d_hist, d_acc);
        hipLaunchKernelGGL(k_dp_merge, dim3((uint32_t)nl), dim3(kDpThreads), 0, ctx->stream, d_off, d_long, d_c, d_class, min_count, (const uint32_t*)d_hist,
                           (const unsigned long long*)d_acc, d_rows);
    }
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

int depth_read_impl(spsp_ctx* ctx, uint32_t min_count, spsp_depth_row* rows, spsp_depth_totals* totals, const uint32_t** d_entry_count) {
    int rc;
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    if (d_entry_count) *d_entry_count = nullptr;
    if (totals) memset(totals, 0, sizeof *totals);
    if (!X.valid || !X.depth) { set_error("%s", kNoDepth); return SPSP_ERR_ARG; }
    const uint32_t R = X.n_ref, E = X.entries, D = X.distinct;
    memset(rows, 0, (size_t)R * sizeof(spsp_depth_row));
    if (min_count == 0) { set_error("depth: min_count is at least 1 (a key no record holds is not found)"); return SPSP_ERR_ARG; }
    if (totals) { totals->record_keys = ctx->dp_record_keys; totals->index_keys = D; }
    if ((rc = ctx->dp_entry.reserve((size_t)E * 4 + 64)) || (rc = ctx->dp_rows.reserve((size_t)R * sizeof(spsp_depth_row)))) return rc;
    if (d_entry_count) *d_entry_count = ctx->dp_entry.as<uint32_t>();
    if (E == 0) { SPSP_HIP(hipStreamSynchronize(ctx->stream)); return SPSP_OK; }   // (an index without a key: nothing is found)
    unsigned long long* d_words = ctx->dp_words.as<unsigned long long>();
    hipEvent_t* ev = nullptr;
    if (ctx->timing) {
        for (hipEvent_t& e : ctx->dp_events) if (!e) SPSP_HIP(hipEventCreate(&e));
        ev = ctx->dp_events;
    }
    if (ev) SPSP_HIP(hipEventRecord(ev[0], ctx->stream));
    if ((rc = depth_launch_entry(ctx, min_count, nullptr))) return rc;
    if (ev) SPSP_HIP(hipEventRecord(ev[1], ctx->stream));
    if ((rc = depth_launch_reduce(ctx, ctx->dp_uniq.as<uint8_t>(), min_count, ctx->dp_rows.as<spsp_depth_row>()))) return rc;
    SPSP_HIP(hipGetLastError());
    if (ev) SPSP_HIP(hipEventRecord(ev[2], ctx->stream));
    unsigned long long words[kDpWords] = {};
    SPSP_HIP(hipMemcpyAsync(rows, ctx->dp_rows.p, (size_t)R * sizeof(spsp_depth_row), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait
    if (ev) {
        for (int i = 0; i < 2; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); ctx->dp_ms[1 + i] += ms; }
    }
    if (totals) { totals->hit_keys = words[kDpwHit]; totals->index_found = (uint32_t)words[kDpwFound]; }
    return SPSP_OK;
}

// depth as a record pass, which serves the profile as well: counters behind the index, a batch's keys added, and at the close --
// in front of the side context's end -- the read and, where asked, the profile.  No per-record rows: nothing to extract from
struct DepthPass : RecordPass {
    spsp_ctx* ctx;
    uint32_t n_ref, min_count;
    std::vector<spsp_depth_row>* rows;
    spsp_depth_totals* totals;
    ProfileAsk* profile;
    uint64_t n_records = 0;
    DepthPass(spsp_ctx* c, uint32_t n, uint32_t min_c, std::vector<spsp_depth_row>* r, spsp_depth_totals* t, ProfileAsk* p)
        : ctx(c), n_ref(n), min_count(min_c), rows(r), totals(t), profile(p) {}
    int on_index() override { return depth_begin_impl(ctx); }
    int on_records(uint32_t n_rec, const uint64_t*) override { n_records += n_rec; return SPSP_OK; }
    int on_batch(const RecordBatch& B) override { return depth_add_impl(ctx, B.mn, B.lo, B.hi, B.key_off[0], B.key_off[B.n_records] - B.key_off[0]); }
    int on_close() override {
        int rc = depth_read_impl(ctx, min_count, rows->data(), totals, nullptr);
        if (!rc && profile) {
            uint64_t n_rows = 0;
            profile->rows.assign(n_ref, spsp_profile_row{});
            rc = profile_impl(ctx, min_count, profile->min_keys, profile->max_rounds, profile->rows.data(), &n_rows, &profile->totals, nullptr);
            profile->rows.resize(rc ? 0 : (size_t)n_rows);
        }
        return rc;
    }
};

int depth_files_impl(spsp_ctx* ctx, const char* const* paths, uint32_t n_ref, const char* const* reads_paths, uint32_t n_reads, uint32_t min_count, int precision,
                     const char* out_prefix, int chatter, double rate, std::vector<spsp_depth_row>* rows, spsp_depth_totals* totals, ProfileAsk* profile) {
    FilesRun run(ctx, paths, n_ref, chatter);
    rows->assign(n_ref, spsp_depth_row{});
    DepthPass pass(ctx, n_ref, min_count, rows, totals, profile);
    RecordsAsk ask;
    ask.records_paths = reads_paths; ask.n_records_paths = n_reads; ask.rate = rate; ask.precision = precision; ask.out_prefix = out_prefix; ask.chatter = chatter;
    RecordsOut out;
    out.want_names = false;
    int rc = records_files_road(run, "depth is", pass, ask, &out);
    const double t1 = out.t1;
    const uint64_t n_records = pass.n_records;
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_depth_csv_host(rows->data(), paths, n_ref, precision, &text, &len))) return rc;
    char* ptext = nullptr; uint64_t plen = 0;              // (both texts stand before either file is written)
    if (profile && (rc = spsp_profile_csv_host(profile->rows.data(), profile->rows.size(), &profile->totals, paths, n_ref, precision, &ptext, &plen))) {
        spsp_free(text);
        return rc;
    }
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_depth.csv.gz", t1))) { spsp_free(ptext); return rc; }
    if (profile && (rc = write_csv_gz(ctx, ptext, plen, out_prefix, "_profile.csv.gz", now_s()))) {
        remove((std::string(out_prefix) + "_depth.csv.gz").c_str());   // (nothing is written on a failure)
        return rc;
    }
    if (!chatter) return rc;
    printf("%llu record(s) against %u reference(s): %llu record key(s), %llu hit key(s), %u of %u index key(s) found\n", (unsigned long long)n_records, n_ref,
           (unsigned long long)totals->record_keys, (unsigned long long)totals->hit_keys, totals->index_found, totals->index_keys);
    if (profile)
        printf("profile: %llu reference(s) named, %u of %u found key(s) assigned, %llu of %llu of their hit key(s)\n", (unsigned long long)profile->rows.size(),
               profile->totals.assigned_keys, profile->totals.found_keys, (unsigned long long)profile->totals.assigned_sum, (unsigned long long)profile->totals.found_sum);
    say_common_rate(run.L, n_ref);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_depth_begin_device(spsp_ctx* ctx) {
    if (!ctx) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return depth_begin_impl(ctx);
}

extern "C" int spsp_depth_add_device(spsp_ctx* ctx, const void* d_q_minimizer, const void* d_q_kmer_lo, const void* d_q_kmer_hi, uint64_t first, uint64_t n_keys) {
    if (!ctx) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return depth_add_impl(ctx, (const uint32_t*)d_q_minimizer, (const uint64_t*)d_q_kmer_lo, (const uint64_t*)d_q_kmer_hi, first, n_keys);
}

extern "C" int spsp_depth_read_device(spsp_ctx* ctx, uint32_t min_count, spsp_depth_row* rows, spsp_depth_totals* totals, const void** d_entry_count) {
    if (d_entry_count) *d_entry_count = nullptr;
    if (!ctx || !rows) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    const uint32_t* d = nullptr;
    const int rc = depth_read_impl(ctx, min_count, rows, totals, &d);
    if (d_entry_count) *d_entry_count = rc == SPSP_OK ? d : nullptr;
    return rc;
}

extern "C" int spsp_depth_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    if (!ctx->dp_add_used.empty()) {
        SPSP_HIP(hipStreamSynchronize(ctx->stream));
        for (auto& ev : ctx->dp_add_used) {
            float t = 0;
            SPSP_HIP(hipEventElapsedTime(&t, ev.first, ev.second));
            ctx->dp_ms[0] += t;
            ctx->dp_add_spare.push_back(ev);
        }
        ctx->dp_add_used.clear();
    }
    for (int i = 0; i < 3; ++i) { ms[i] = ctx->dp_ms[i]; ctx->dp_ms[i] = 0; }
    return SPSP_OK;
}

extern "C" int spsp_depth_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* const* reads_paths, uint32_t n_reads, uint32_t min_count,
                                int precision, const char* out_prefix, int chatter, double rate, spsp_depth_row** rows, spsp_depth_totals* totals) {
    if (rows) *rows = nullptr;
    spsp_depth_totals mine{};
    if (totals) *totals = mine;
    if (!ctx || !index_paths || !reads_paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (uint32_t f = 0; f < n_reads; ++f) if (!reads_paths[f]) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    if (n_reads == 0) { set_error("depth takes at least one reads file"); return SPSP_ERR_ARG; }
    if (min_count == 0) { set_error("depth: min_count is at least 1 (a key no record holds is not found)"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_depth_row> got;
    int rc;
    if ((rc = depth_files_impl(ctx, index_paths, n_ref, reads_paths, n_reads, min_count, precision, out_prefix, chatter, rate, &got, &mine, nullptr))) return rc;
    if (totals) *totals = mine;
    if (rows && (rc = give_rows(got, rows))) return rc;
    return SPSP_OK;
}
