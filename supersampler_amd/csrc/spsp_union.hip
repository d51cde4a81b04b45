// The union of two record batches on the GPU: per record r the keys of A_r and B_r together, each once, sorted (not in the
// reference, which has no record passes).  The rule is in include/spsp.h ("paired records"): A and B are the two mates' key lists
// of a batch of pairs, and the result is what spsp_classify_device / spsp_taxonomy_device take as the pairs' keys.
//
// Both sides come sorted per record by (minimizer, kmer_hi, kmer_lo) and distinct, so a key's place in its record's union is its
// own rank plus its rank in the other side, less what the two share below it.  A lane per KEY, never per record: a contig pair of
// 10^6 keys among a million read pairs costs its keys.  A lane's only loops are binary searches (its record among the offsets, its
// key in the other side's stretch) and at most three popcounts.
//   k_un_flag     a workgroup per kUnTile entries of B, then the workgroups over A's entries.  A lane of B: its record, its key's
//                 lower bound in that record's stretch of A (kept: at[j], counted from A's first entry), whether A holds the key;
//                 the wave's ballot of "new" keys is one 64-bit word, the workgroup's count one word of the scan.  Every lane, of A
//                 and of B, checks that its key lies above its predecessor in the record: the least (side, record) that fails is
//                 left in the call's flag word by one atomicMin.
//   scan          launch_scan_u32 over the tiles' counts.  new_before(j) = the new keys among B's first j entries: the tile's
//                 offset, the popcounts of the tile's words in front of j's, and a masked one.
//   k_un_offsets  a lane per record boundary: off[r] = |A_0..r-1| + new_before(B's entries in front of record r).  B's entries
//                 are in record order, so the one prefix over B is every record's prefix at once.
//   k_un_write    the same grid as k_un_flag.  Entry i of A goes to i + new_before(the lower bound of its key in B_r); a new entry
//                 j of B to at[j] + new_before(j).  Both are below |A| + new(B): no store leaves the output whatever the keys hold.
// Bound: every key read twice and written once, 12 or 20 bytes each, beside the searches' reads, which stay in L2 for records of
// reads.  One host wait, at the end, which brings the offsets, the flag word and the total.  No workgroup waits for another.
#include <algorithm>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

static_assert(kUnTile == kUnThreads && kUnThreads % 64 == 0, "a tile of B is one workgroup's entries: a ballot word per wave");
constexpr uint32_t kUnWaves = kUnThreads / 64;

// the first entry of K in [lo, hi) that is not below (mn, hi_w, lo_w)
template <bool HAS_HI>
__device__ __forceinline__ uint64_t un_lower_bound(const SortedKeys& K, uint64_t lo, uint64_t hi, uint32_t mn, uint64_t hi_w, uint64_t lo_w) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys_less<HAS_HI>(K, mid, mn, hi_w, lo_w)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the new keys among B's entries [0, j), j <= n_b
__device__ __forceinline__ uint32_t un_new_before(const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ tile_off, uint64_t j) {
    const uint64_t t = j / kUnTile, wj = j >> 6;
    uint32_t v = tile_off[t];
    for (uint64_t w = t * kUnWaves; w < wj; ++w) v += (uint32_t)__popcll(mask[w]);   // (three words at the most)
    if (j & 63ull) v += (uint32_t)__popcll(mask[wj] & ((1ull << (j & 63ull)) - 1ull));
    return v;
}

// entry e of side `side` (0: A, 1: B) in record r must lie above entry e - 1 where that is in the record too
template <bool HAS_HI>
__device__ __forceinline__ void un_check_order(const SortedKeys& K, const uint64_t* __restrict__ off, uint32_t r, uint64_t e, uint32_t mn, uint64_t hi, uint64_t lo,
                                               unsigned long long side, unsigned long long* __restrict__ word) {
    if (e > off[r] && !keys_less<HAS_HI>(K, e - 1, mn, hi, lo)) atomicMin(word, side << 32 | r);
}

template <bool HAS_HI>
__global__ __launch_bounds__(kUnThreads) void k_un_flag(SortedKeys A, SortedKeys B, const uint64_t* __restrict__ a_off, const uint64_t* __restrict__ b_off,
                                                        uint32_t n_rec, uint32_t g_b, unsigned long long* __restrict__ word, uint32_t* __restrict__ at,
                                                        unsigned long long* __restrict__ mask, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_cnt[kUnWaves];
    const uint64_t a0 = a_off[0], b0 = b_off[0], n_a = a_off[n_rec] - a0, n_b = b_off[n_rec] - b0;
    if (blockIdx.x >= g_b) {                               // (uniform) A's entries: the order alone
        const uint64_t i = (uint64_t)(blockIdx.x - g_b) * kUnThreads + threadIdx.x;
        if (i >= n_a) return;
        const uint64_t e = a0 + i;
        un_check_order<HAS_HI>(A, a_off, sorted_sketch_of(a_off, 0, n_rec, e), e, A.mn[e], HAS_HI ? A.hi[e] : 0ull, A.lo[e], 0ull, word);
        return;
    }
    const uint64_t j = (uint64_t)blockIdx.x * kUnTile + threadIdx.x;
    bool is_new = false;
    if (j < n_b) {
        const uint64_t e = b0 + j;
        const uint32_t mn = B.mn[e];
        const uint64_t lo = B.lo[e], hi = HAS_HI ? B.hi[e] : 0ull;
        const uint32_t r = sorted_sketch_of(b_off, 0, n_rec, e);
        un_check_order<HAS_HI>(B, b_off, r, e, mn, hi, lo, 1ull, word);
        const uint64_t end = a_off[r + 1], lb = un_lower_bound<HAS_HI>(A, a_off[r], end, mn, hi, lo);
        at[j] = (uint32_t)(lb - a0);
        is_new = !(lb < end && pv_same<HAS_HI>(A, lb, mn, hi, lo));
    }
    const unsigned long long ballot = __ballot(is_new);
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    if (lane == 0u) { mask[(uint64_t)blockIdx.x * kUnWaves + wid] = ballot; s_cnt[wid] = (uint32_t)__popcll(ballot); }   // (every wave: a word behind n_b is 0)
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kUnWaves; ++w) all += s_cnt[w];
        tile_cnt[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kUnThreads) void k_un_offsets(const uint64_t* __restrict__ a_off, const uint64_t* __restrict__ b_off, uint32_t n_rec,
                                                           const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ tile_off,
                                                           uint64_t* __restrict__ off) {
    const uint64_t r = (uint64_t)blockIdx.x * kUnThreads + threadIdx.x;
    if (r > n_rec) return;
    off[r] = (a_off[r] - a_off[0]) + un_new_before(mask, tile_off, b_off[r] - b_off[0]);
}

template <bool HAS_HI>
__global__ __launch_bounds__(kUnThreads) void k_un_write(SortedKeys A, SortedKeys B, const uint64_t* __restrict__ a_off, const uint64_t* __restrict__ b_off,
                                                         uint32_t n_rec, uint32_t g_b, const uint32_t* __restrict__ at,
                                                         const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ tile_off,
                                                         uint32_t* __restrict__ o_mn, uint64_t* __restrict__ o_lo, uint64_t* __restrict__ o_hi) {
    const uint64_t a0 = a_off[0], b0 = b_off[0], n_a = a_off[n_rec] - a0, n_b = b_off[n_rec] - b0;
    uint32_t mn;
    uint64_t lo, hi = 0ull, pos;
    if (blockIdx.x >= g_b) {                               // (uniform)
        const uint64_t i = (uint64_t)(blockIdx.x - g_b) * kUnThreads + threadIdx.x;
        if (i >= n_a) return;
        const uint64_t e = a0 + i;
        mn = A.mn[e]; lo = A.lo[e];
        if (HAS_HI) hi = A.hi[e];
        const uint32_t r = sorted_sketch_of(a_off, 0, n_rec, e);
        pos = i + un_new_before(mask, tile_off, un_lower_bound<HAS_HI>(B, b_off[r], b_off[r + 1], mn, hi, lo) - b0);   // (<= n_a - 1 + new(B))
    } else {
        const uint64_t j = (uint64_t)blockIdx.x * kUnTile + threadIdx.x;
        if (j >= n_b || !((mask[j >> 6] >> (j & 63ull)) & 1ull)) return;
        const uint64_t e = b0 + j;
        mn = B.mn[e]; lo = B.lo[e];
        if (HAS_HI) hi = B.hi[e];
        pos = (uint64_t)at[j] + un_new_before(mask, tile_off, j);   // (at <= n_a, and j itself is new: <= n_a + new(B) - 1)
    }
    o_mn[pos] = mn; o_lo[pos] = lo;
    if (HAS_HI) o_hi[pos] = hi;
}

// the work area carved once: the flag word | the three offset arrays | at[] | the ballot words | the tiles' counts | their scan
struct UnWork {
    unsigned long long* word;
    uint64_t *a_off, *b_off, *off;
    unsigned long long* mask;
    uint32_t *at, *tile_cnt, *tile_off;
    static size_t bytes(uint32_t n_rec, uint64_t n_b, uint32_t g_b) {
        return 8 + (size_t)3 * ((size_t)n_rec + 1) * 8 + ((size_t)g_b * kUnWaves + 1) * 8 + ((size_t)n_b + 2 * (size_t)g_b + 4) * 4;
    }
    UnWork(void* base, uint32_t n_rec, uint64_t n_b, uint32_t g_b)
        : word(reinterpret_cast<unsigned long long*>(base)), a_off(reinterpret_cast<uint64_t*>(word + 1)), b_off(a_off + n_rec + 1), off(b_off + n_rec + 1),
          mask(reinterpret_cast<unsigned long long*>(off + n_rec + 1)), at(reinterpret_cast<uint32_t*>(mask + (size_t)g_b * kUnWaves + 1)), tile_cnt(at + n_b),
          tile_off(tile_cnt + g_b) {}
};

}  // namespace

int records_union_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* a_mn, const uint64_t* a_lo, const uint64_t* a_hi, const uint64_t* h_a_off, const uint32_t* b_mn,
                       const uint64_t* b_lo, const uint64_t* b_hi, const uint64_t* h_b_off, uint32_t n_rec, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi,
                       uint64_t* h_off) {
    int rc;
    *out_mn = nullptr; *out_lo = nullptr; *out_hi = nullptr;
    if (n_rec <= 0xfffffff0u) for (uint32_t r = 0; r <= n_rec; ++r) h_off[r] = 0;
    else h_off[0] = 0;
    // (the order of record_call_front: the record count, the offsets, the key count, then the arrays against k)
    if (k < 1 || k > 63) { set_error("k=%u out of range 1..63", k); return SPSP_ERR_ARG; }
    if (n_rec > 0xfffffff0u) { set_error("too many records for one call (%u)", n_rec); return SPSP_ERR_OVERFLOW; }
    for (int side = 0; side < 2; ++side) {
        const uint64_t* o = side ? h_b_off : h_a_off;
        for (uint32_t r = 0; r < n_rec; ++r)
            if (o[r + 1] < o[r]) { set_error("union: record offsets must not decrease (side %c, record %u)", side ? 'B' : 'A', r); return SPSP_ERR_ARG; }
    }
    const uint64_t n_a = h_a_off[n_rec] - h_a_off[0], n_b = h_b_off[n_rec] - h_b_off[0];
    if (h_a_off[n_rec] > 0xfffffff0ull || h_b_off[n_rec] > 0xfffffff0ull || n_a + n_b > 0xfffffff0ull) {
        set_error("too many record keys for one call");
        return SPSP_ERR_OVERFLOW;
    }
    const bool has_hi = k > 32;
    if ((n_a && (!a_mn || !a_lo)) || (n_b && (!b_mn || !b_lo))) { set_error("NULL key array"); return SPSP_ERR_ARG; }
    if ((n_a && (a_hi != nullptr) != has_hi) || (n_b && (b_hi != nullptr) != has_hi)) {
        set_error("union: k = %u takes its keys %s kmer_hi (k %s 32), side %c comes %s it", k, has_hi ? "with" : "without", has_hi ? ">" : "<=",
                  (n_a && (a_hi != nullptr) != has_hi) ? 'A' : 'B', has_hi ? "without" : "with");
        return SPSP_ERR_ARG;
    }
    const uint32_t g_b = (uint32_t)((n_b + kUnTile - 1) / kUnTile), g_a = (uint32_t)((n_a + kUnThreads - 1) / kUnThreads);
    const size_t room = (size_t)std::max<uint64_t>(n_a + n_b, 1);
    if ((rc = ctx->un_work.reserve(UnWork::bytes(n_rec, n_b, g_b))) || (rc = ctx->un_mn.reserve(room * 4)) || (rc = ctx->un_lo.reserve(room * 8)) ||
        (has_hi && (rc = ctx->un_hi.reserve(room * 8)))) return rc;
    const UnWork W(ctx->un_work.p, n_rec, n_b, g_b);
    uint32_t* o_mn = ctx->un_mn.as<uint32_t>();
    uint64_t *o_lo = ctx->un_lo.as<uint64_t>(), *o_hi = has_hi ? ctx->un_hi.as<uint64_t>() : nullptr;
    hipStream_t st = ctx->stream;
    SPSP_HIP(hipMemsetAsync(W.word, 0xff, 8, st));
    SPSP_HIP(hipMemcpyAsync(W.a_off, h_a_off, ((size_t)n_rec + 1) * 8, hipMemcpyHostToDevice, st));   // (the caller's: alive until the wait)
    SPSP_HIP(hipMemcpyAsync(W.b_off, h_b_off, ((size_t)n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    const SortedKeys A{a_mn, a_lo, a_hi}, B{b_mn, b_lo, b_hi};
    RecordClock& clock = ctx->un_clock;
    if ((rc = clock.mark(ctx, 0))) return rc;
    if (g_a + g_b) {
        if (has_hi) hipLaunchKernelGGL(k_un_flag<true>, dim3(g_a + g_b), dim3(kUnThreads), 0, st, A, B, (const uint64_t*)W.a_off, (const uint64_t*)W.b_off, n_rec,
                                       g_b, W.word, W.at, W.mask, W.tile_cnt);
        else hipLaunchKernelGGL(k_un_flag<false>, dim3(g_a + g_b), dim3(kUnThreads), 0, st, A, B, (const uint64_t*)W.a_off, (const uint64_t*)W.b_off, n_rec, g_b,
                                W.word, W.at, W.mask, W.tile_cnt);
        SPSP_HIP(hipGetLastError());
    }
    if ((rc = clock.mark(ctx, 1)) || (rc = launch_scan_u32(ctx, W.tile_cnt, W.tile_off, g_b, ctx->h_scalar + kHsUnNew)) || (rc = clock.mark(ctx, 2))) return rc;
    hipLaunchKernelGGL(k_un_offsets, dim3((uint32_t)(((uint64_t)n_rec + kUnThreads) / kUnThreads)), dim3(kUnThreads), 0, st, (const uint64_t*)W.a_off,
                       (const uint64_t*)W.b_off, n_rec, (const unsigned long long*)W.mask, (const uint32_t*)W.tile_off, W.off);
    SPSP_HIP(hipGetLastError());
    if ((rc = clock.mark(ctx, 3))) return rc;
    if (g_a + g_b) {
        if (has_hi) hipLaunchKernelGGL(k_un_write<true>, dim3(g_a + g_b), dim3(kUnThreads), 0, st, A, B, (const uint64_t*)W.a_off, (const uint64_t*)W.b_off, n_rec,
                                       g_b, (const uint32_t*)W.at, (const unsigned long long*)W.mask, (const uint32_t*)W.tile_off, o_mn, o_lo, o_hi);
        else hipLaunchKernelGGL(k_un_write<false>, dim3(g_a + g_b), dim3(kUnThreads), 0, st, A, B, (const uint64_t*)W.a_off, (const uint64_t*)W.b_off, n_rec, g_b,
                                (const uint32_t*)W.at, (const unsigned long long*)W.mask, (const uint32_t*)W.tile_off, o_mn, o_lo, o_hi);
        SPSP_HIP(hipGetLastError());
    }
    if ((rc = clock.mark(ctx, 4))) return rc;
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsUnBad, W.word, 8, hipMemcpyDeviceToHost, st));
    SPSP_HIP(hipMemcpyAsync(h_off, W.off, ((size_t)n_rec + 1) * 8, hipMemcpyDeviceToHost, st));
    SPSP_HIP(hipStreamSynchronize(st));                    // the one wait
    if (clock.on)
        for (int i = 0; i < 4; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, clock.ev[i], clock.ev[i + 1])); clock.ms[i] += ms; }
    const uint64_t bad = ctx->h_scalar[kHsUnBad];
    if (bad != ~0ull) {
        for (uint32_t r = 0; r <= n_rec; ++r) h_off[r] = 0;
        set_error("union: the keys of side %c, record %u are not strictly increasing by (minimizer, kmer_hi, kmer_lo)", (bad >> 32) ? 'B' : 'A', (uint32_t)bad);
        return SPSP_ERR_ARG;
    }
    if (h_off[n_rec] != n_a + ctx->h_scalar[kHsUnNew]) {   // (never: the offsets and the total come from one scan)
        for (uint32_t r = 0; r <= n_rec; ++r) h_off[r] = 0;
        set_error("union: the offsets end at %llu, the keys at %llu (the key arrays changed during the call?)", (unsigned long long)h_off[n_rec],
                  (unsigned long long)(n_a + ctx->h_scalar[kHsUnNew]));
        return SPSP_ERR_ARG;
    }
    *out_mn = o_mn; *out_lo = o_lo; *out_hi = o_hi;
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_records_union_device(spsp_ctx* ctx, uint32_t k, const void* d_a_min, const void* d_a_lo, const void* d_a_hi, const uint64_t* h_a_off,
                                         const void* d_b_min, const void* d_b_lo, const void* d_b_hi, const uint64_t* h_b_off, uint32_t n_records, void** d_min,
                                         void** d_lo, void** d_hi, uint64_t* h_off) {
    if (d_min) *d_min = nullptr;
    if (d_lo) *d_lo = nullptr;
    if (d_hi) *d_hi = nullptr;
    if (!ctx || !h_a_off || !h_b_off || !d_min || !d_lo || !d_hi || !h_off) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint32_t* mn = nullptr;
    uint64_t *lo = nullptr, *hi = nullptr;
    const int rc = records_union_impl(ctx, k, (const uint32_t*)d_a_min, (const uint64_t*)d_a_lo, (const uint64_t*)d_a_hi, h_a_off, (const uint32_t*)d_b_min,
                                      (const uint64_t*)d_b_lo, (const uint64_t*)d_b_hi, h_b_off, n_records, &mn, &lo, &hi, h_off);
    *d_min = mn; *d_lo = lo; *d_hi = hi;
    return rc;
}

extern "C" int spsp_union_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    ctx->un_clock.hand_out(ms);
    return SPSP_OK;
}
