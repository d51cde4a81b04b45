// Classification on the GPU: which references each record of a sequence file belongs to (not in the reference, whose end product
// is the two n x n matrices).
//
// The index is a collection as every collection pass takes it: references 0 .. R-1 back to back, each sorted by (minimizer, kmer_hi,
// kmer_lo), with key sets K_j.  A record r has a set Q_r of distinct keys, in any order, in arrays of the caller's.
//   shared(r, j) = |Q_r n K_j|        hit_keys(r) = #{x in Q_r : some K_j holds x}
// Reference j passes for r when shared >= min_keys and shared * den >= num * |Q_r|; the matches of r are its best min(top, passing)
// passing references by the 64-bit word shared << 32 | (0xffffffff - j): more shared keys first, the lower number among equals.  The
// order is total, so nothing below depends on which lane met what first.  Integers only.
//
// The index, built once (spsp_classify_index_device): key_major_build (spsp_accumulation.hip) -- the prevalence table filled with
// claimers, and the key-major CSR: key_start[0 .. D] and the 16-bit holder numbers, list behind list.  The scatter has spent the
// slots' counters as cursors; a lookup goes slot -> claimer entry -> key_no -> key_start[kn], key_start[kn + 1] -> list[].
// Per batch of records (spsp_classify_device), one chain of launches whatever the records are:
//   k_cf_probe   a lane per record key: the probe sequence of k_pv_read, a miss at the first free slot; kn[e] = the key's number + 1
//                (0: nobody holds it).  The lane's h goes to its record's work and 1 to its hit keys: one add per wave where the
//                wave sits inside one record (a contig), one per lane with a hit otherwise (reads: a few lanes per record).
//                Bound: one random 8-byte slot read and one 20-byte key read per key -- HBM latency under full occupancy.
//   k_rec_route  (spsp_device.h) a lane per record: no work -> its row is written there (CfEmptyRow); work <= kCfSmallWork -> the
//                queue of the small form; else the queue of the large form.  The queues' order is a race and no result depends on
//                it.  No host wait: the two forms below are launched with grids sized by the records there can be and stride
//                over what the queues hold.
//   k_cf_small   a wave per record: the holder numbers of all its keys gathered into the wave's 4 KiB of LDS (long lists by the
//                whole wave, as in the large form), sorted there by a bitonic network (wave_sort_lds), and every run of equal
//                numbers counted by a binary search for its start; the runs are offered 64 at a time to the kept matches.
//                Bound: LDS traffic of the sort, (log2 P)^2 / 2 steps over P <= 1 024 words.
//   k_cf_large   a workgroup per record with one 32-bit counter per reference: in LDS while 4 R bytes fit beside the kept matches
//                (R <= kCfLdsRefs), in a row of HBM per workgroup beyond.  A wave takes 64 keys; a lane walks its own list, lists
//                of more than kCfListCut holders are walked by the whole wave (coalesced: a contig against its species has
//                h = R on every key).  Then every wave offers its share of the counters, and wave 0 merges the eight kept lists.
//                Bound: Sum h atomic adds, on LDS at the LDS atomic rate, beyond kCfLdsRefs on L2.
// Kept matches: one 64-bit word per lane, best first.  A chunk of 64 candidates that holds nothing in front of the top-th kept word
// is dropped with one ballot; else it is sorted by the register bitonic network of spsp_neighbours.hip and merged with the kept 64.
// The host waits once per batch, at the end.  No workgroup ever waits for another one.
// This file is also the home of what the record passes share on the host (DESIGN "What the record passes share"): the front of a
// record call, its device arrays and clock, the records of a text in batches, and the road of the four file drivers.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kCfWaves = kCfThreads / 64, kCfLargeWaves = kCfLargeThreads / 64;
static_assert(kCfThreads == kRouteThreads && kCfWaves == kRecordWaves, "the record calls' route and wave-form grids");

__device__ __forceinline__ unsigned long long cf_word(uint32_t shared, uint32_t ref) { return (unsigned long long)shared << 32 | (0xffffffffu - ref); }

// one compare-exchange with the lane `j` away: the lane keeps the larger word (front) or the smaller one
__device__ __forceinline__ void cf_exchange(unsigned long long& v, uint32_t j, bool front) {
    const unsigned long long o = __shfl_xor(v, (int)j);
    if (front ? o > v : o < v) v = o;
}

// kept: the best 64 so far, best first, one per lane (0: none).  v: one candidate per lane (0: none).  Words of real candidates are
// distinct (a reference is offered once) and only the first `top` kept words are ever read: a chunk that holds nothing in front of
// the top-th one changes nothing
__device__ __forceinline__ void cf_offer(unsigned long long& kept, unsigned long long v, uint32_t lane, uint32_t top) {
    if (!__any(v > __shfl(kept, (int)(top - 1u)))) return;
#pragma unroll
    for (uint32_t k = 2; k <= 64u; k <<= 1)
#pragma unroll
        for (uint32_t j = k >> 1; j; j >>= 1) cf_exchange(v, j, ((lane & j) == 0) == ((lane & k) == 0));
    // kept (best first) against the chunk reversed: the larger of every pair -- the best 64 of the 128, as a bitonic run
    const unsigned long long o = __shfl(v, (int)(63u - lane));
    if (o > kept) kept = o;
#pragma unroll
    for (uint32_t j = 32; j; j >>= 1) cf_exchange(kept, j, (lane & j) == 0);
}

// Q: the records' keys, entries [off[0], off[n_rec]); K, tbl, key_no, key_start: the index (first: its first entry, n_index: its entries)
template <bool HAS_HI>
__global__ __launch_bounds__(kCfThreads) void k_cf_probe(SortedKeys Q, const uint64_t* __restrict__ off, uint32_t n_rec, SortedKeys K, uint64_t first,
                                                         uint32_t n_index, const unsigned long long* __restrict__ tbl, uint32_t log2cap,
                                                         const uint32_t* __restrict__ key_no, const uint32_t* __restrict__ key_start,
                                                         uint32_t* __restrict__ kn_out, unsigned long long* __restrict__ work, uint32_t* __restrict__ hit) {
    const uint64_t q0 = off[0], n_keys = off[n_rec] - q0;
    const uint64_t i = (uint64_t)blockIdx.x * kCfThreads + threadIdx.x;
    const bool valid = i < n_keys;
    uint32_t kn = 0, h = 0, rec = 0xffffffffu;
    if (valid) {
        const uint64_t e = q0 + i;
        const uint32_t mn = Q.mn[e];
        const uint64_t lo = Q.lo[e], hi = HAS_HI ? Q.hi[e] : 0ull;
        const uint64_t at = pv_find<HAS_HI>(K, first, n_index, tbl, log2cap, mn, hi, lo);
        if (at != ~0ull) {
            const uint32_t number = key_no[at];
            kn = number + 1u;
            h = key_start[number + 1u] - key_start[number];
        }
        kn_out[i] = kn;
        rec = sorted_sketch_of(off, 0, n_rec, e);
    }
    // the record's work and hit keys.  Entries are in record order: first and last lane in one record = the whole wave in it
    const uint32_t r0 = __shfl(rec, 0), r63 = __shfl(rec, 63);
    if (r0 == r63) {                                       // (uniform.  A wave of lanes beyond the keys: 0xffffffff, nothing to add)
        unsigned long long w = h;
        uint32_t c = kn != 0u;
#pragma unroll
        for (int d = 32; d; d >>= 1) { w += __shfl_xor(w, d); c += __shfl_xor(c, d); }   // (one loop for both, not two wave_sum: measured)
        if ((threadIdx.x & 63u) == 0u && c != 0u) { atomicAdd(&work[r0], w); atomicAdd(&hit[r0], c); }
    } else if (kn != 0u) {
        atomicAdd(&work[rec], (unsigned long long)h);
        atomicAdd(&hit[rec], 1u);
    }
}

// rec[r]: keys, hit_keys, passing, listed.  The row of a record without work, which the route kernel writes
struct CfEmptyRow {
    __device__ void operator()(uint4* __restrict__ rec, uint32_t r, uint32_t keys) const { rec[r] = make_uint4(keys, 0u, 0u, 0u); }
};

// a wave per queued record; kn, and the entries of off, count from the first record key
__global__ __launch_bounds__(kCfThreads) void k_cf_small(const uint64_t* __restrict__ off, const uint32_t* __restrict__ kn_of, const uint32_t* __restrict__ hit,
                                                         const uint32_t* __restrict__ key_start, const uint16_t* __restrict__ list,
                                                         const uint32_t* __restrict__ q_small, uint32_t* __restrict__ words, uint32_t top,
                                                         uint32_t min_keys, uint32_t num, uint32_t den, uint4* __restrict__ rec, spsp_classify_hit* __restrict__ hits) {
    __shared__ uint32_t s_all[kCfWaves][kCfSmallWork];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t* s = s_all[wid];
    const uint32_t n_small = words[kRqSmall];
    const uint64_t q0 = off[0];
    for (uint64_t q = (uint64_t)blockIdx.x * kCfWaves + wid; q < n_small; q += (uint64_t)gridDim.x * kCfWaves) {   // (uniform per wave)
        const uint32_t r = q_small[q];
        const uint64_t a = off[r] - q0, z = off[r + 1] - q0;
        const uint32_t keys = (uint32_t)(z - a);
        // the holder numbers of all the record's keys, list behind list
        uint32_t W = 0;
        bool fits = true;
        for (uint64_t base = a; base < z; base += 64ull) {
            const uint64_t i = base + lane;
            const uint32_t kn = i < z ? kn_of[i] : 0u;
            const uint32_t ls = kn ? key_start[kn - 1u] : 0u, len = kn ? key_start[kn] - ls : 0u;
            const uint32_t incl = wave_prefix_incl(len, lane);
            const uint32_t total = __shfl(incl, 63);
            if (total > kCfSmallWork - W) { fits = false; break; }   // (never: the route sent a record of this much work elsewhere.  Uniform)
            const uint32_t at = W + incl - len;
            if (len <= kCfListCut)
                for (uint32_t j = 0; j < len; ++j) s[at + j] = list[ls + j];
            wave_long_lists(len > kCfListCut, ls, len, [=](int l, uint32_t s0, uint32_t n0) {
                const uint32_t a0 = __shfl(at, l);
                for (uint32_t j = lane; j < n0; j += 64u) s[a0 + j] = list[s0 + j];
            });
            W += total;
        }
        if (!fits) { if (lane == 0u) atomicOr(words + kRqBad, 1u); continue; }
        uint32_t P = 64;
        while (P < W) P <<= 1;
        for (uint32_t i = W + lane; i < P; i += 64u) s[i] = 0xffffffffu;
        wave_sort_lds(s, P, lane);
        // every run of one number is a reference with shared = the run's length: its last place less the first place of its number
        unsigned long long kept = 0ull;
        uint32_t passing = 0;
        for (uint32_t base = 0; base < W; base += 64u) {   // (uniform)
            const uint32_t i = base + lane;
            unsigned long long v = 0ull;
            if (i < W) {
                const uint32_t ref = s[i];
                if (i + 1u == W || s[i + 1u] != ref) {
                    const uint32_t shared = i + 1u - lds_lower_bound(s, i, ref);
                    if (passes_threshold(shared, keys, min_keys, num, den)) v = cf_word(shared, ref);
                }
            }
            passing += (uint32_t)__popcll(__ballot(v != 0ull));
            cf_offer(kept, v, lane, top);
        }
        wave_lds_sync();                                   // (the words are read: the next record may overwrite them)
        const uint32_t listed = passing < top ? passing : top;
        if (lane < listed) {
            spsp_classify_hit o;
            o.reference = 0xffffffffu - (uint32_t)kept; o.shared = (uint32_t)(kept >> 32);
            hits[(uint64_t)r * top + lane] = o;
        }
        if (lane == 0u) rec[r] = make_uint4(keys, hit[r], passing, listed);
    }
}

// a workgroup per queued record.  LDS: [IN_LDS: R_pad counters |] the waves' kept matches | the passing count.  rows: !IN_LDS, a row
// of R_pad counters per workgroup
template <bool IN_LDS>
__global__ __launch_bounds__(kCfLargeThreads) void k_cf_large(const uint64_t* __restrict__ off, const uint32_t* __restrict__ kn_of, const uint32_t* __restrict__ hit,
                                                              const uint32_t* __restrict__ key_start, const uint16_t* __restrict__ list,
                                                              const uint32_t* __restrict__ q_large, const uint32_t* __restrict__ words, uint32_t R,
                                                              uint32_t R_pad, uint32_t* __restrict__ rows, uint32_t top, uint32_t min_keys, uint32_t num,
                                                              uint32_t den, uint4* __restrict__ rec, spsp_classify_hit* __restrict__ hits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    uint32_t* cnt = IN_LDS ? s_mem : rows + (size_t)blockIdx.x * R_pad;
    unsigned long long* s_kept = reinterpret_cast<unsigned long long*>(s_mem + (IN_LDS ? R_pad : 0u));
    uint32_t* s_pass = reinterpret_cast<uint32_t*>(s_kept + kCfLargeWaves * 64u);
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t n_large = words[kRqLarge];
    const uint64_t q0 = off[0];
    for (uint64_t q = blockIdx.x; q < n_large; q += gridDim.x) {   // (uniform per workgroup)
        const uint32_t r = q_large[q];
        const uint64_t a = off[r] - q0, z = off[r + 1] - q0;
        const uint32_t keys = (uint32_t)(z - a);
        // (the rows in device memory are added to at L2: they are cleared and read there as well, past this CU's L1)
        for (uint32_t j = threadIdx.x; j < R; j += kCfLargeThreads) {
            if (IN_LDS) cnt[j] = 0u;
            else __hip_atomic_store(cnt + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x == 0u) *s_pass = 0u;
        __syncthreads();
        for (uint64_t base = a + (uint64_t)wid * 64ull; base < z; base += (uint64_t)kCfLargeWaves * 64ull) {   // (uniform per wave)
            const uint64_t i = base + lane;
            const uint32_t kn = i < z ? kn_of[i] : 0u;
            const uint32_t ls = kn ? key_start[kn - 1u] : 0u, len = kn ? key_start[kn] - ls : 0u;
            if (len <= kCfListCut)
                for (uint32_t j = 0; j < len; ++j) { const uint32_t sk = list[ls + j]; if (sk < R) atomicAdd(&cnt[sk], 1u); }
            wave_long_lists(len > kCfListCut, ls, len, [=](int, uint32_t s0, uint32_t n0) {
                for (uint32_t j = lane; j < n0; j += 64u) { const uint32_t sk = list[s0 + j]; if (sk < R) atomicAdd(&cnt[sk], 1u); }
            });
        }
        __syncthreads();
        unsigned long long kept = 0ull;
        uint32_t passing = 0;
        for (uint32_t base = wid * 64u; base < R; base += kCfLargeThreads) {   // (uniform per wave)
            const uint32_t j = base + lane;
            const uint32_t c = j >= R ? 0u : IN_LDS ? cnt[j] : __hip_atomic_load(cnt + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long v = c != 0u && passes_threshold(c, keys, min_keys, num, den) ? cf_word(c, j) : 0ull;
            passing += (uint32_t)__popcll(__ballot(v != 0ull));
            cf_offer(kept, v, lane, top);
        }
        s_kept[wid * 64u + lane] = kept;
        if (lane == 0u && passing) atomicAdd(s_pass, passing);
        __syncthreads();
        if (wid == 0u) {
            for (uint32_t w = 1; w < kCfLargeWaves; ++w) {
                const unsigned long long o = s_kept[w * 64u + 63u - lane];   // (best first there: reversed here)
                if (!__any(o > kept)) continue;
                if (o > kept) kept = o;
#pragma unroll
                for (uint32_t j = 32; j; j >>= 1) cf_exchange(kept, j, (lane & j) == 0);
            }
            const uint32_t all = *s_pass, listed = all < top ? all : top;
            if (lane < listed) {
                spsp_classify_hit o;
                o.reference = 0xffffffffu - (uint32_t)kept; o.shared = (uint32_t)(kept >> 32);
                hits[(uint64_t)r * top + lane] = o;
            }
            if (lane == 0u) rec[r] = make_uint4(keys, hit[r], all, listed);
        }
        __syncthreads();                                   // (the counters and the kept words are read: the next record clears them)
    }
}

}  // namespace

int classify_index_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n_ref) {
    int rc;
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    KeysShape shape;
    if ((rc = sorted_keys_front(ctx, "classification reads", k, d_mn, d_lo, d_hi, h_sk_off, n_ref, &shape))) return rc;
    spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    X = spsp_ctx::ClassifyIndex{};
    if (shape.all_keys) {
        KeyMajor km;
        if ((rc = key_major_build(ctx, shape.has_hi, d_mn, d_lo, d_hi, h_sk_off, n_ref, kAcCut, &km))) return rc;
        SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsCfBad, km.words, 8, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // the index call's wait
        const uint64_t flags = ctx->h_scalar[kHsCfBad];
        if ((uint32_t)flags) { set_error("sketch keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)"); return SPSP_ERR_ARG; }
        if (flags >> 32) { set_error("classification: a key's list could not be placed (the key arrays changed during the call?)"); return SPSP_ERR_ARG; }
        X.key_no = km.key_no; X.key_start = km.key_start; X.list = km.list; X.entries = km.entries;
    }
    X.has_hi = shape.has_hi; X.n_ref = n_ref; X.first = shape.first;
    X.mn = d_mn; X.lo = d_lo; X.hi = d_hi;
    X.off_host.assign(h_sk_off, h_sk_off + n_ref + 1);
    X.valid = true;                                        // (behind the build: the table fill in it drops whatever index there was)
    return SPSP_OK;
}

int classify_probe_launch(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, const uint64_t* d_off, uint32_t n_rec,
                          uint64_t all_keys, uint32_t* d_kn, unsigned long long* d_work, uint32_t* d_hit) {
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    const SortedKeys Q{q_mn, q_lo, q_hi}, K{X.mn, X.lo, X.hi};
    const unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
    const uint32_t gp = (uint32_t)((all_keys + kCfThreads - 1) / kCfThreads);
    if (X.has_hi) hipLaunchKernelGGL(k_cf_probe<true>, dim3(gp), dim3(kCfThreads), 0, ctx->stream, Q, d_off, n_rec, K, X.first, X.entries, d_tbl,
                                     ctx->pv_log2cap, X.key_no, X.key_start, d_kn, d_work, d_hit);
    else hipLaunchKernelGGL(k_cf_probe<false>, dim3(gp), dim3(kCfThreads), 0, ctx->stream, Q, d_off, n_rec, K, X.first, X.entries, d_tbl,
                            ctx->pv_log2cap, X.key_no, X.key_start, d_kn, d_work, d_hit);
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

int refuse_no_index(const char* pass) {
    set_error("%s: the context holds no index (spsp_classify_index_device first; a prevalence, select, accumulation or groups call replaces it)", pass);
    return SPSP_ERR_ARG;
}

int record_keys_check(const spsp_ctx* ctx, const char* pass, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, uint64_t n_keys) {
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    if (n_keys && (!q_mn || !q_lo)) { set_error("NULL key array"); return SPSP_ERR_ARG; }
    if (n_keys && (q_hi != nullptr) != X.has_hi) {
        set_error("%s: the index was built %s kmer_hi (k %s 32), the records come %s it", pass, X.has_hi ? "with" : "without", X.has_hi ? ">" : "<=",
                  q_hi ? "with" : "without");
        return SPSP_ERR_ARG;
    }
    return SPSP_OK;
}

int record_call_front(const spsp_ctx* ctx, const char* pass, bool needs_taxonomy, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi,
                      const uint64_t* h_rec_off, uint32_t n_rec, uint64_t* all_keys) {
    if (n_rec > 0xfffffff0u) { set_error("too many records for one call (%u)", n_rec); return SPSP_ERR_OVERFLOW; }
    for (uint32_t r = 0; r < n_rec; ++r)
        if (h_rec_off[r + 1] < h_rec_off[r]) { set_error("record offsets must not decrease (record %u)", r); return SPSP_ERR_ARG; }
    if (h_rec_off[n_rec] > 0xfffffff0ull) { set_error("too many record keys for one call"); return SPSP_ERR_OVERFLOW; }
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    if (!X.valid) return refuse_no_index(pass);
    if (needs_taxonomy && !X.taxonomy) {
        set_error("taxonomy: the index holds no taxonomy (spsp_taxonomy_index_device first; it ends with the index it was attached to)");
        return SPSP_ERR_ARG;
    }
    *all_keys = h_rec_off[n_rec] - h_rec_off[0];
    return record_keys_check(ctx, pass, q_mn, q_lo, q_hi, *all_keys);
}

int RecordWork::reserve(spsp_ctx* ctx, uint32_t n, uint64_t keys, size_t row) {
    int rc;
    n_rec = n; all_keys = keys; row_bytes = row;
    const size_t work_bytes = (size_t)n * 8;
    if ((rc = ctx->cf_off.reserve(((size_t)n + 1) * 8)) || (rc = ctx->cf_kn.reserve((size_t)keys * 4)) || (rc = ctx->cf_work.reserve(work_bytes + (size_t)n * 4)) ||
        (rc = ctx->cf_queue.reserve(64 + (size_t)2 * n * 4)) || (rc = ctx->cf_rec.reserve((size_t)n * row))) return rc;
    off = ctx->cf_off.as<uint64_t>();
    kn = ctx->cf_kn.as<uint32_t>();
    work = ctx->cf_work.as<unsigned long long>();
    hit = reinterpret_cast<uint32_t*>(ctx->cf_work.as<uint8_t>() + work_bytes);
    words = ctx->cf_queue.as<uint32_t>();
    q_small = words + 16;
    q_large = q_small + n;
    rec = ctx->cf_rec.as<uint4>();
    g_route = (uint32_t)(((uint64_t)n + kRouteThreads - 1) / kRouteThreads);
    g_small = (uint32_t)std::min<uint64_t>(((uint64_t)n + kRecordWaves - 1) / kRecordWaves, (uint64_t)std::max(ctx->n_cu, 1) * 8u);
    return SPSP_OK;
}

int RecordWork::upload(spsp_ctx* ctx, const uint64_t* h_rec_off) {
    SPSP_HIP(hipMemcpyAsync(off, h_rec_off, ((size_t)n_rec + 1) * 8, hipMemcpyHostToDevice, ctx->stream));   // (the caller's: alive until the wait)
    return SPSP_OK;
}

int RecordWork::clear(spsp_ctx* ctx) {
    SPSP_HIP(hipMemsetAsync(work, 0, (size_t)n_rec * 12, ctx->stream));   // (the hit keys sit behind the work)
    SPSP_HIP(hipMemsetAsync(words, 0, kRqWords * 4, ctx->stream));
    SPSP_HIP(hipMemsetAsync(rec, 0, (size_t)n_rec * row_bytes, ctx->stream));
    return SPSP_OK;
}

int RecordWork::read_back(spsp_ctx* ctx, std::vector<uint32_t>* rows) {
    rows->resize((size_t)n_rec * (row_bytes / 4));         // (in front of the copies: the device is still at work while the host clears these)
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsCfBad, words + kRqBad, 4, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(rows->data(), rec, rows->size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    return SPSP_OK;
}

int RecordWork::wait(spsp_ctx* ctx, RecordClock& clock, bool* fitted) {
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait
    if (clock.on)
        for (int i = 0; i < 4; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, clock.ev[i], clock.ev[i + 1])); clock.ms[i] += ms; }
    *fitted = (uint32_t)ctx->h_scalar[kHsCfBad] == 0u;
    return SPSP_OK;
}

int RecordClock::mark(spsp_ctx* ctx, int i) {
    if (i == 0 && (on = ctx->timing))                      // spsp_timing_enable: events between the launches (the pass's *_stage_ms call)
        for (hipEvent_t& e : ev) if (!e) SPSP_HIP(hipEventCreate(&e));
    if (on) SPSP_HIP(hipEventRecord(ev[i], ctx->stream));
    return SPSP_OK;
}

void RecordClock::hand_out(double* out) {
    for (int i = 0; i < 4; ++i) { out[i] = ms[i]; ms[i] = 0; }
}

int classify_device_impl(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, const uint64_t* h_rec_off, uint32_t n_rec,
                         uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den, spsp_classify_record* records, spsp_classify_hit* hits) {
    int rc;
    // (what is zeroed in front of the refusals: the records' counts always, the hits once `top` says how many there are)
    for (uint32_t r = 0; r < n_rec; ++r) records[r].keys = records[r].hit_keys = records[r].passing = records[r].listed = 0;
    if (n_rec && top >= 1 && top <= kCfMaxTop) memset(hits, 0, (size_t)n_rec * top * sizeof(spsp_classify_hit));
    uint64_t all_keys = 0;
    if ((rc = classify_check_args(top, min_keys, num, den)) || (rc = record_call_front(ctx, "classification", false, q_mn, q_lo, q_hi, h_rec_off, n_rec, &all_keys)))
        return rc;
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    for (uint32_t r = 0; r < n_rec; ++r) records[r].keys = (uint32_t)(h_rec_off[r + 1] - h_rec_off[r]);   // (length is the caller's)
    if (n_rec == 0 || all_keys == 0 || X.entries == 0) return SPSP_OK;   // (no record, no record key or no reference key: nothing is shared)

    const uint32_t R = X.n_ref, R_pad = (R + 3u) & ~3u;
    const bool in_lds = R <= kCfLdsRefs;
    const int n_cu = std::max(ctx->n_cu, 1);
    const size_t lds = kCfLargeFixedLds + (in_lds ? (size_t)R_pad * 4 : 0), hits_bytes = (size_t)n_rec * top * sizeof(spsp_classify_hit);
    const uint32_t large_per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(2048 / kCfLargeThreads, kAcLdsBytes / lds));
    const uint32_t g_large = (uint32_t)std::min<uint64_t>(n_rec, (uint64_t)n_cu * (in_lds ? large_per_cu : 1u));
    RecordWork W;
    if ((rc = W.reserve(ctx, n_rec, all_keys, 16)) || (rc = ctx->cf_hits.reserve(hits_bytes)) ||
        (!in_lds && (rc = ctx->cf_rows.reserve((size_t)g_large * R_pad * 4)))) return rc;
    spsp_classify_hit* d_hits = ctx->cf_hits.as<spsp_classify_hit>();
    uint32_t* d_rows = in_lds ? nullptr : ctx->cf_rows.as<uint32_t>();
    if ((rc = W.upload(ctx, h_rec_off)) || (rc = W.clear(ctx))) return rc;
    SPSP_HIP(hipMemsetAsync(d_hits, 0, hits_bytes, ctx->stream));
    RecordClock& clock = ctx->cf_clock;
    if ((rc = clock.mark(ctx, 0)) || (rc = classify_probe_launch(ctx, q_mn, q_lo, q_hi, W.off, n_rec, all_keys, W.kn, W.work, W.hit)) || (rc = clock.mark(ctx, 1)))
        return rc;
    hipLaunchKernelGGL((k_rec_route<unsigned long long, CfEmptyRow>), dim3(W.g_route), dim3(kRouteThreads), 0, ctx->stream, (const uint64_t*)W.off, n_rec,
                       (const unsigned long long*)W.work, (unsigned long long)kCfSmallWork, W.words, W.q_small, W.q_large, W.rec, CfEmptyRow{});
    if ((rc = clock.mark(ctx, 2))) return rc;
    hipLaunchKernelGGL(k_cf_small, dim3(W.g_small), dim3(kCfThreads), 0, ctx->stream, (const uint64_t*)W.off, (const uint32_t*)W.kn, (const uint32_t*)W.hit,
                       X.key_start, X.list, (const uint32_t*)W.q_small, W.words, top, min_keys, num, den, W.rec, d_hits);
    if ((rc = clock.mark(ctx, 3))) return rc;
    if (in_lds) {
        if ((rc = lds_opt_in(ctx, &k_cf_large<true>, kAcLdsBytes))) return rc;
        hipLaunchKernelGGL(k_cf_large<true>, dim3(g_large), dim3(kCfLargeThreads), lds, ctx->stream, (const uint64_t*)W.off, (const uint32_t*)W.kn,
                           (const uint32_t*)W.hit, X.key_start, X.list, (const uint32_t*)W.q_large, (const uint32_t*)W.words, R, R_pad, d_rows, top, min_keys,
                           num, den, W.rec, d_hits);
    } else {
        hipLaunchKernelGGL(k_cf_large<false>, dim3(g_large), dim3(kCfLargeThreads), lds, ctx->stream, (const uint64_t*)W.off, (const uint32_t*)W.kn,
                           (const uint32_t*)W.hit, X.key_start, X.list, (const uint32_t*)W.q_large, (const uint32_t*)W.words, R, R_pad, d_rows, top, min_keys,
                           num, den, W.rec, d_hits);
    }
    SPSP_HIP(hipGetLastError());
    if ((rc = clock.mark(ctx, 4))) return rc;
    std::vector<uint32_t> got;
    bool fitted = false;
    if ((rc = W.read_back(ctx, &got))) return rc;
    SPSP_HIP(hipMemcpyAsync(hits, d_hits, hits_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = W.wait(ctx, clock, &fitted))) return rc;
    if (!fitted) {
        set_error("classification: a record's holders did not fit the form it was routed to (the key arrays changed during the call?)");
        memset(hits, 0, hits_bytes);
        return SPSP_ERR_ARG;
    }
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint32_t* g = got.data() + (size_t)r * 4;
        records[r].keys = g[0]; records[r].hit_keys = g[1]; records[r].passing = g[2]; records[r].listed = g[3];
    }
    return SPSP_OK;
}

// seam[b] = the first super-k-mer of the stream (which is in record order) whose record is want[b] or behind it
__global__ void k_cf_seams(const spsp_superkmer* __restrict__ sk, uint64_t n_sk, const uint32_t* __restrict__ want, uint32_t n, uint64_t* __restrict__ seam) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const uint32_t w = want[b];
    uint64_t lo = 0, hi = n_sk;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (sk[mid].rec < w) lo = mid + 1; else hi = mid; }
    seam[b] = lo;
}

// every batch's stretch of the super-k-mer stream: batch b = records [want[b], want[b + 1]) -> super-k-mers [seam[b], seam[b + 1]).  One launch, one wait
static int batch_seams(spsp_ctx* ctx, const spsp_superkmer* d_sk, uint64_t n_sk, const std::vector<uint32_t>& want, std::vector<uint64_t>* seam) {
    int rc;
    const uint32_t n = (uint32_t)want.size();
    seam->assign(n, 0);
    if ((rc = ctx->cf_off.reserve((size_t)n * 12 + 64))) return rc;
    uint64_t* d_seam = ctx->cf_off.as<uint64_t>();
    uint32_t* d_want = reinterpret_cast<uint32_t*>(d_seam + n);
    SPSP_HIP(hipMemcpyAsync(d_want, want.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_cf_seams, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_sk, n_sk, (const uint32_t*)d_want, n, d_seam);
    SPSP_HIP(hipGetLastError());
    SPSP_HIP(hipMemcpyAsync(seam->data(), d_seam, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));
    return SPSP_OK;
}

// One text, ingested and scanned once on its side context: what the unpaired form has one of and the paired form two.  open: the
// upload, the ingest, the header count held against the REAL records, the windows expansion where there is one, the scan, the
// two stage times, the records' offsets on the host (one wait).  seams: every batch's stretch of the stream.  keys_begin /
// keys_end: a batch's key extraction queued and collected, so that two sides' extractions overlap on their streams
struct TextSide {
    spsp_ctx* side = nullptr;
    spsp_params ps{};
    uint8_t* d_bases = nullptr;
    uint64_t* d_off = nullptr;
    uint64_t n_text = 0, n_bases = 0, n_sk = 0;
    uint32_t n_rec = 0;
    spsp_superkmer* d_sk = nullptr;
    std::vector<uint64_t> rec_off, seam, key_off;
    std::vector<uint32_t> first_rec;

    // t0: where the ingest's stage time begins (the unpaired form counts the reading of the names in).  n_names: null, or the
    // header lines the host read.  windows: null, or the run that takes the real records' offsets and first_win
    int open(spsp_ctx* ctx, const spsp_params* p, const uint8_t* text, uint64_t text_bytes, const char* path, double t0, const size_t* n_names, WindowsRun* windows) {
        int rc;
        double t1;
        n_text = text_bytes;
        const bool fastq = n_text && text[0] == '@';
        if ((rc = side->i_text.reserve((size_t)n_text + 64))) return rc;
        if (n_text) SPSP_HIP(hipMemcpyAsync(side->i_text.p, text, (size_t)n_text, hipMemcpyHostToDevice, side->stream));
        const bool packed = ingest_packs(p);
        FastqLayout fq;
        if (fastq) fastq_tail(text, n_text, &fq.content_end, &fq.blank_tail);
        if ((rc = clean_device_impl(side, side->i_text.as<uint8_t>(), n_text, &d_bases, &n_bases, &d_off, &n_rec, packed, fastq ? &fq : nullptr))) return rc;
        if (n_names && *n_names != n_rec) {                // (held against the REAL records, whatever the passes see)
            set_error("'%s': %zu header line(s) on the host, %u record(s) on the device", path, *n_names, n_rec);
            return SPSP_ERR_FORMAT;
        }
        if (windows) {
            // the expansion, between the ingest and the scan: from here on the windows are the records (their bases in the side
            // context's windows buffer, in the form the ingest wrote).  The real records' offsets and first_win stay with the run
            windows->rec_off.assign((size_t)n_rec + 1, 0);
            windows->first_win.assign((size_t)n_rec + 1, 0);
            windows->d_text = side->i_text.as<uint8_t>(); windows->n_text = n_text;   // (the upload above: read again by the lift behind the last batch)
            windows->d_bases = d_bases; windows->n_bases = n_bases; windows->packed = packed;   // (the ingest's buffer: it stays as it is until the side context ends)
            SPSP_HIP(hipMemcpyAsync(windows->rec_off.data(), d_off, windows->rec_off.size() * 8, hipMemcpyDeviceToHost, side->stream));   // (the expansion waits)
            uint8_t* w_bases = nullptr; uint64_t* w_off = nullptr; uint64_t w_n = 0, n_win = 0;
            if ((rc = records_windows_impl(side, d_bases, n_bases, d_off, n_rec, p->k, windows->window, packed, &w_bases, &w_n, &w_off, windows->first_win.data(), &n_win)))
                return rc;
            d_bases = w_bases; n_bases = w_n; d_off = w_off; n_rec = (uint32_t)n_win;
        }
        t1 = now_s(); ctx->stages.ingest_s += t1 - t0; t0 = t1;
        ps = *p;
        if (packed) ps.flags |= SPSP_SCAN_PACKED_INPUT;
        if ((rc = scan_device_impl(side, &ps, d_bases, n_bases, d_off, n_rec, &d_sk, &n_sk))) return rc;
        t1 = now_s(); ctx->stages.scan_s += t1 - t0;
        rec_off.assign((size_t)n_rec + 1, 0);
        SPSP_HIP(hipMemcpyAsync(rec_off.data(), d_off, rec_off.size() * 8, hipMemcpyDeviceToHost, side->stream));
        SPSP_HIP(hipStreamSynchronize(side->stream));
        return SPSP_OK;
    }
    // (the extraction takes any record range of the scan: it looks its genomes' super-k-mers up by record number.  It gets the
    // batch's own stretch of the stream all the same, so that a batch costs its records and not the file's)
    int seams(const std::vector<uint32_t>& bounds) { return n_rec ? batch_seams(side, d_sk, n_sk, bounds, &seam) : (int)SPSP_OK; }
    int keys_begin(uint32_t r0, uint32_t batch, size_t b) {
        first_rec.resize((size_t)batch + 1);
        for (uint32_t g = 0; g <= batch; ++g) first_rec[g] = r0 + g;
        key_off.assign((size_t)batch + 1, 0);
        return spsp_sketch_keys_device_begin(side, &ps, d_bases, n_bases, d_off, d_sk + seam[b], seam[b + 1] - seam[b], first_rec.data(), batch, 0);
    }
    int keys_end(void** k) { return spsp_sketch_keys_device_end(side, &k[0], &k[1], &k[2], key_off.data()); }
};

// behind the last batch (every batch's rows are on the host: each record call waits), with the texts still in the side contexts'
// buffers: the pass makes ONE flag or bin vector from its rows, and every text is cut by it
static int cut_texts(spsp_ctx* ctx, uint32_t k, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out, TextSide* S, int n_sides) {
    int rc;
    const uint32_t n_rec = S[0].n_rec;
    if (ask.mode == kRmWindows) {
        // the rows are the windows': their calls are the split's bins.  Smoothing, segments, mosaic and the texts follow here, where
        // the side context still holds the real records' bases for the segments' text
        const size_t n_win = pass.n_rows();
        std::vector<uint32_t> call(n_win ? n_win : 1, 0), keys(call.size(), 0), hit_keys(call.size(), 0), support(call.size(), 0);
        uint32_t n_bins = 0;
        if ((rc = pass.bins(ask.what, (uint32_t)n_win, call.data(), &n_bins))) return rc;
        for (size_t w = 0; w < n_win; ++w) pass.window_addends(w, &keys[w], &hit_keys[w], &support[w]);
        if ((rc = spsp_wait_stream(S[0].side, ctx))) return rc;
        return windows_tail(S[0].side, &out->windows, ask, k, call, keys, hit_keys, support, n_bins, out->names, pass.bin_names(), pass.last_name());
    }
    if (ask.mode == kRmSplit) {
        std::vector<uint32_t> bin(n_rec ? n_rec : 1, SPSP_SPLIT_DROP);
        uint32_t n_bins = 0;
        if ((rc = pass.bins(ask.what, n_rec, bin.data(), &n_bins))) return rc;
        for (int s = 0; s < n_sides; ++s)
            if ((rc = out->extract[s].split_text(S[s].side, S[s].side->i_text.as<uint8_t>(), S[s].n_text, n_rec, bin.data(), n_bins))) return rc;
    } else if (ask.mode == kRmExtract) {
        std::vector<uint8_t> keep(n_rec ? n_rec : 1, 0);
        if ((rc = pass.keep_flags(ask.what, n_rec, keep.data()))) return rc;
        for (int s = 0; s < n_sides; ++s)
            if ((rc = out->extract[s].on_text(S[s].side, S[s].side->i_text.as<uint8_t>(), S[s].n_text, n_rec, keep.data()))) return rc;
    }
    return SPSP_OK;
}

// the records of n_sides texts (1: a records file; 2: the two mates' files, record p of either being the two mates of pair p --
// the rule: include/spsp.h, "paired records"), each on its side context, through the pass batch by batch.  The paired form holds
// the record counts and the names against each other in front of everything else, hands on_records the pairs' summed base
// offsets, and per batch queues the two key extractions on the two sides' streams before it collects either, makes their union
// on ctx and hands that to on_batch as the unpaired form hands a batch's keys
static int records_text_batches(spsp_ctx* ctx, spsp_ctx* const* side, int n_sides, const spsp_params* p, const uint8_t* const* text, const uint64_t* n_text,
                                const char* const* path, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out) {
    int rc;
    const double t0 = now_s();
    const bool paired = n_sides == 2;
    std::vector<std::string> mate_names[2];
    std::vector<std::string>* names[2] = {paired ? &mate_names[0] : &out->names, &mate_names[1]};
    if (paired || out->want_names)
        for (int s = 0; s < n_sides; ++s) record_names_host(text[s], n_text[s], n_text[s] && text[s][0] == '@', names[s]);
    if (paired) {
        if (mate_names[0].size() != mate_names[1].size()) {
            set_error("paired files must hold as many records: '%s' has %zu, '%s' has %zu", path[0], mate_names[0].size(), path[1], mate_names[1].size());
            return SPSP_ERR_FORMAT;
        }
        const size_t n = mate_names[0].size();
        std::vector<const char*> p1(n), p2(n);
        for (size_t r = 0; r < n; ++r) { p1[r] = mate_names[0][r].c_str(); p2[r] = mate_names[1][r].c_str(); }
        char* common = nullptr; uint64_t bad = 0;
        if ((rc = spsp_pairs_names_host(p1.data(), p2.data(), n, &common, &bad))) return rc;
        out->names.clear();
        for (size_t r = 0, at = 0; r < n; ++r) { out->names.emplace_back(common + at); at += out->names.back().size() + 1; }
        spsp_free(common);
    }
    TextSide S[2];
    for (int s = 0; s < n_sides; ++s) {
        const size_t n_names = names[s]->size();
        S[s].side = side[s];
        if ((rc = S[s].open(ctx, p, text[s], n_text[s], path[s], paired ? now_s() : t0, paired || out->want_names ? &n_names : nullptr,
                            ask.mode == kRmWindows ? &out->windows : nullptr))) return rc;
    }
    const uint32_t n_rec = S[0].n_rec;
    if (paired) {
        std::vector<uint64_t> sum_off((size_t)n_rec + 1);
        for (uint32_t r = 0; r <= n_rec; ++r) sum_off[r] = S[0].rec_off[r] + S[1].rec_off[r];
        rc = pass.on_records(n_rec, sum_off.data());
    } else rc = pass.on_records(n_rec, S[0].rec_off.data());
    if (rc) return rc;
    const std::vector<uint32_t> bounds = records_batch_bounds(n_rec);
    for (int s = 0; s < n_sides; ++s)
        if ((rc = S[s].seams(bounds))) return rc;
    std::vector<uint64_t> union_off;
    for (size_t b = 0; b + 1 < bounds.size(); ++b) {
        const uint32_t r0 = bounds[b], batch = bounds[b + 1] - r0;
        void* km[2][3] = {};
        for (int s = 0; s < n_sides; ++s)                  // (the last batch's keys, or its union, have been read)
            if ((rc = spsp_wait_stream(side[s], ctx)) || (rc = S[s].keys_begin(r0, batch, b))) return rc;
        for (int s = 0; s < n_sides; ++s)
            if ((rc = S[s].keys_end(km[s])) || (rc = spsp_wait_stream(ctx, side[s]))) return rc;
        RecordBatch B{r0, batch, (const uint32_t*)km[0][0], (const uint64_t*)km[0][1], (const uint64_t*)km[0][2], S[0].key_off.data()};
        if (paired) {
            uint32_t* u_mn = nullptr;
            uint64_t *u_lo = nullptr, *u_hi = nullptr;
            union_off.assign((size_t)batch + 1, 0);
            if ((rc = records_union_impl(ctx, p->k, B.mn, B.lo, B.hi, B.key_off, (const uint32_t*)km[1][0], (const uint64_t*)km[1][1], (const uint64_t*)km[1][2],
                                         S[1].key_off.data(), batch, &u_mn, &u_lo, &u_hi, union_off.data()))) return rc;
            B = RecordBatch{r0, batch, u_mn, u_lo, u_hi, union_off.data()};
        }
        if ((rc = pass.on_batch(B))) return rc;
    }
    return cut_texts(ctx, p->k, pass, ask, out, S, n_sides);
}

int records_files_road(FilesRun& run, const char* what_is, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out) {
    spsp_ctx* ctx = run.ctx;
    int rc = run.load(ask.rate);
    if (!rc) rc = run.refuse_k_eq_m(rc, what_is);
    double rec_rate = run.L.ds_rate;                       // the records are scanned at ONE threshold: mixed rates need a rate, as -S
    if (!rc) rc = sketches_out_rate(run.L, run.paths, run.n, &rec_rate);
    if ((rc = run.begin(rc))) return rc;
    const DecodedKeys& keys = run.keys;
    rc = run.decode();
    if (!rc) rc = classify_index_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), run.n);
    if (!rc) rc = pass.on_index();
    if (!rc) {
        spsp_ctx* side[2] = {nullptr, nullptr};
        spsp_params p{};
        p.k = keys.k; p.m = keys.m; p.threshold = spsp_threshold_host(keys.k, keys.m, rec_rate); p.abundance = 1; p.flags = 0;
        for (uint32_t f = 0; !rc && !ask.mates_path && f < ask.n_records_paths; ++f) {
            uint8_t* text = nullptr; uint64_t n_text = 0;
            if (!(rc = spsp_read_file_host(ask.records_paths[f], &text, &n_text)) && (side[0] || !(rc = spsp_create(ctx->device, nullptr, &side[0]))) &&
                !(rc = spsp_wait_stream(side[0], ctx)))    // (the last file's keys have been read)
                rc = records_text_batches(ctx, side, 1, &p, &text, &n_text, &ask.records_paths[f], pass, ask, out);
            spsp_free(text);
        }
        if (!rc && ask.mates_path) {                       // the paired form: records_paths[0] and mates_path on a side context each
            const char* path[2] = {ask.records_paths[0], ask.mates_path};
            uint8_t* text[2] = {nullptr, nullptr}; uint64_t n_text[2] = {0, 0};
            if (!(rc = spsp_read_file_host(path[0], &text[0], &n_text[0])) && !(rc = spsp_read_file_host(path[1], &text[1], &n_text[1])) &&
                !(rc = spsp_create(ctx->device, nullptr, &side[0])) && !(rc = spsp_create(ctx->device, nullptr, &side[1])))
                rc = records_text_batches(ctx, side, 2, &p, text, n_text, path, pass, ask, out);
            spsp_free(text[0]); spsp_free(text[1]);
        }
        if (!rc) rc = pass.on_close();
        (void)hipStreamSynchronize(ctx->stream);           // (what on_batch queued reads the side contexts' key arrays)
        for (spsp_ctx* s : side)
            if (s) { (void)hipStreamSynchronize(s->stream); spsp_destroy(s); }
    }
    out->t1 = run.end();
    return rc;
}

// what a driver writes for its extraction: the split's files and manifest, the one file of extract[0].write, or the two files of a
// paired run and one line for both
static int extract_write(spsp_ctx* ctx, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out) {
    ExtractRun *extract = &out->extract[0], *mates = ask.mates_path ? &out->extract[1] : nullptr;
    if (ask.mode == kRmSplit) return split_write(ctx, extract, mates, pass.bin_names(), pass.last_name(), ask.out_prefix, ask.chatter);
    if (!mates) return extract->write(ctx, ask.out_prefix, ask.chatter);
    int rc;
    if ((rc = extract->write(ctx, ask.out_prefix, 0)) || (rc = mates->write(ctx, ask.out_prefix, 0)) || !ask.chatter) return rc;
    printf("extract %s: %llu of %llu pair(s) kept, %llu + %llu byte(s) written to %s_extract_1 and _extract_2\n", extract->what, (unsigned long long)extract->n_kept,
           (unsigned long long)extract->n_rec, (unsigned long long)extract->out.size(), (unsigned long long)mates->out.size(), ask.out_prefix);
    fflush(stdout);
    return SPSP_OK;
}

int record_files_run(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out) {
    FilesRun run(ctx, index_paths, n_ref, ask.chatter);
    for (ExtractRun& e : out->extract) { e.what = ask.what; e.gz = ask.gz; }
    if (ask.mates_path) { out->extract[0].tag = "_1"; out->extract[1].tag = "_2"; }
    out->windows.window = ask.window;
    int rc;
    if ((rc = records_files_road(run, "classification is", pass, ask, out))) return rc;
    if (ask.mode == kRmWindows) {
        // the texts were made behind the last batch; the two windowed CSVs take the per-record CSVs' place
        if ((rc = windows_files(ctx, &out->windows, ask, out->t1))) return rc;
    } else if ((rc = pass.write_rows(run, ask, out->names, out->t1)) || (ask.mode != kRmPlain && (rc = extract_write(ctx, pass, ask, out)))) return rc;
    if (ask.chatter) {
        if (ask.mode != kRmWindows) pass.say_rows(run, ask);
        say_common_rate(run.L, n_ref);
        fflush(stdout);
    }
    return SPSP_OK;
}

int record_files_entry(const RecordFront& front, RecordPass& pass, const RecordsAsk& ask, RecordsOut* out) {
    int rc;
    if ((rc = record_files_check_args(front, ask))) return rc;
    SPSP_HIP(hipSetDevice(front.ctx->device));
    if ((rc = pass.prelude(ask))) return rc;
    return record_files_run(front.ctx, front.index_paths, front.n_ref, pass, ask, out);
}

// classify as a record pass: the rows of all records (windows) on the host, a batch's call into its stretch of them
struct ClassifyPass : RecordPass {
    spsp_ctx* ctx;
    const char* const* paths;
    uint32_t n_ref, top, min_keys, num, den;
    std::vector<spsp_classify_record> recs;
    std::vector<spsp_classify_hit> hits;
    explicit ClassifyPass(const RecordFront& f) : ctx(f.ctx), paths(f.index_paths), n_ref(f.n_ref), top(f.top), min_keys(f.min_keys), num(f.num), den(f.den) {}
    int on_records(uint32_t n_rec, const uint64_t* rec_off) override {
        recs.assign(n_rec, spsp_classify_record{});
        hits.assign((size_t)n_rec * top, spsp_classify_hit{});
        for (uint32_t r = 0; r < n_rec; ++r) recs[r].length = rec_off[r + 1] - rec_off[r];
        return SPSP_OK;
    }
    int on_batch(const RecordBatch& B) override {
        return classify_device_impl(ctx, B.mn, B.lo, B.hi, B.key_off, B.n_records, top, min_keys, num, den, recs.data() + B.first_record,
                                    hits.data() + (size_t)B.first_record * top);
    }
    int keep_flags(const char* what, uint32_t n, uint8_t* keep) override { return spsp_extract_flags_classify_host(what, recs.data(), hits.data(), n, top, n_ref, keep); }
    int bins(const char* what, uint32_t n, uint32_t* bin, uint32_t* n_bins) override {
        return spsp_split_bins_classify_host(what, recs.data(), hits.data(), n, top, n_ref, bin, n_bins);
    }
    void window_addends(size_t w, uint32_t* keys, uint32_t* hit_keys, uint32_t* support) override {
        *keys = recs[w].keys; *hit_keys = recs[w].hit_keys;
        *support = recs[w].listed ? hits[w * top].shared : 0u;
    }
    const char* const* bin_names() override { return paths; }   // (the names the summary prints: the references' paths)
    const char* last_name() override { return "unmatched"; }
    size_t n_rows() override { return recs.size(); }
    int write_rows(FilesRun&, const RecordsAsk& ask, const std::vector<std::string>& names, double t1) override {
        int rc;
        std::vector<const char*> name_ptr(names.size());
        for (size_t r = 0; r < names.size(); ++r) name_ptr[r] = names[r].c_str();
        char* text = nullptr; uint64_t len = 0;
        if ((rc = spsp_classify_csv_host(recs.data(), hits.data(), recs.size(), name_ptr.data(), paths, n_ref, top, ask.precision, &text, &len))) return rc;
        if ((rc = write_csv_gz(ctx, text, len, ask.out_prefix, "_classify.csv.gz", t1))) return rc;
        const double t2 = now_s();
        if ((rc = spsp_classify_summary_csv_host(recs.data(), hits.data(), recs.size(), paths, n_ref, top, &text, &len))) return rc;
        return write_csv_gz(ctx, text, len, ask.out_prefix, "_classify_summary.csv.gz", t2);
    }
    void say_rows(FilesRun&, const RecordsAsk& ask) override {
        uint64_t with = 0;
        for (const spsp_classify_record& r : recs) with += r.listed != 0;
        printf(ask.mates_path ? "%zu pair(s) against %u reference(s): %llu with a match\n" : "%zu record(s) against %u reference(s): %llu with a match\n", recs.size(), n_ref,
               (unsigned long long)with);
    }
};

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_classify_index_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi,
                                          const uint64_t* h_sk_off, uint32_t n_ref) {
    if (!ctx || !h_sk_off) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return classify_index_impl(ctx, k, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n_ref);
}

extern "C" int spsp_classify_device(spsp_ctx* ctx, const void* d_q_minimizer, const void* d_q_kmer_lo, const void* d_q_kmer_hi, const uint64_t* h_rec_off,
                                    uint32_t n_records, uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den, spsp_classify_record* records,
                                    spsp_classify_hit* hits) {
    if (!ctx || !h_rec_off || (n_records && (!records || !hits))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return classify_device_impl(ctx, (const uint32_t*)d_q_minimizer, (const uint64_t*)d_q_kmer_lo, (const uint64_t*)d_q_kmer_hi, h_rec_off, n_records, top,
                                min_keys, num, den, records, hits);
}

// spsp_classify_files, _extract, _paired and _split behind the filling of their ask: the outputs cleared, the front and the
// driver, the rows handed out
static int classify_files_entry(const RecordFront& front, const RecordsAsk& ask, spsp_classify_record** records, spsp_classify_hit** hits, uint64_t* n_records,
                                uint64_t* n_kept, uint64_t* bytes_out) {
    if (records) *records = nullptr;
    if (hits) *hits = nullptr;
    if (n_records) *n_records = 0;
    if (n_kept) *n_kept = 0;
    if (bytes_out) *bytes_out = 0;
    ClassifyPass pass(front);
    RecordsOut out;
    if (const int rc = record_files_entry(front, pass, ask, &out)) return rc;
    if (n_kept) *n_kept = out.n_kept(ask);
    if (bytes_out) *bytes_out = out.bytes_out();
    if (n_records) *n_records = pass.recs.size();
    const RowsGift gifts[] = {{(void**)records, pass.recs.data(), pass.recs.size() * sizeof(spsp_classify_record)},
                              {(void**)hits, pass.hits.data(), pass.hits.size() * sizeof(spsp_classify_hit)}};
    return give_rows_all(gifts, 2);
}

extern "C" int spsp_classify_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                   uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                   spsp_classify_record** records, spsp_classify_hit** hits, uint64_t* n_records) {
    return classify_files_entry({ctx, index_paths, nullptr, false, false, n_ref, top, min_keys, num, den},
                                records_ask(&records_path, nullptr, kRmPlain, nullptr, 1, 0, precision, out_prefix, chatter, rate), records, hits, n_records, nullptr, nullptr);
}

extern "C" int spsp_classify_files_extract(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top,
                                           uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                           spsp_classify_record** records, spsp_classify_hit** hits, uint64_t* n_records, const char* what, int gz,
                                           uint64_t* n_kept, uint64_t* bytes_out) {
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }   // (in front of the clearing: DESIGN "What the record file drivers share")
    return classify_files_entry({ctx, index_paths, nullptr, false, false, n_ref, top, min_keys, num, den},
                                records_ask(&records_path, nullptr, kRmExtract, what, gz, 0, precision, out_prefix, chatter, rate), records, hits, n_records, n_kept, bytes_out);
}

extern "C" int spsp_classify_files_paired(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path,
                                          uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter,
                                          double rate, const char* what, int gz, spsp_classify_record** records, spsp_classify_hit** hits, uint64_t* n_records,
                                          uint64_t* n_kept, uint64_t* bytes_out) {
    return classify_files_entry({ctx, index_paths, nullptr, false, true, n_ref, top, min_keys, num, den},
                                records_ask(&records_path, mates_path, what ? kRmExtract : kRmPlain, what, gz, 0, precision, out_prefix, chatter, rate), records, hits,
                                n_records, n_kept, bytes_out);
}

extern "C" int spsp_classify_files_split(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path,
                                         uint32_t top, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter,
                                         double rate, const char* what, int gz, spsp_classify_record** records, spsp_classify_hit** hits, uint64_t* n_records,
                                         uint64_t* n_bins_written, uint64_t* bytes_out) {
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }   // (likewise)
    return classify_files_entry({ctx, index_paths, nullptr, false, false, n_ref, top, min_keys, num, den},
                                records_ask(&records_path, mates_path, kRmSplit, what, gz, 0, precision, out_prefix, chatter, rate), records, hits, n_records,
                                n_bins_written, bytes_out);
}

extern "C" int spsp_classify_files_raw(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                            uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window,
                                            const char* what, spsp_classify_record** rows, spsp_classify_hit** hits, uint64_t* n_windows, uint32_t** first_win,
                                            uint64_t* n_records, spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth,
                                            const char* segments_what, uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out, int raw,
                                       uint64_t** raw_begin, uint64_t** raw_end, uint64_t* bed_bytes) {
    if (rows) *rows = nullptr;
    if (hits) *hits = nullptr;
    if (first_win) *first_win = nullptr;
    if (segments) *segments = nullptr;
    if (mosaic) *mosaic = nullptr;
    if (raw_begin) *raw_begin = nullptr;
    if (raw_end) *raw_end = nullptr;
    for (uint64_t* n : {n_windows, n_records, n_segments, n_changed, n_written, bytes_out, bed_bytes}) if (n) *n = 0;
    const RecordFront front{ctx, index_paths, nullptr, false, false, n_ref, top, min_keys, num, den};
    ClassifyPass pass(front);
    RecordsOut out;
    RecordsAsk ask = records_ask(&records_path, nullptr, kRmWindows, what, gz, window, precision, out_prefix, chatter, rate);
    ask.smooth = smooth; ask.segments_what = segments_what; ask.segments_min = segments_min; ask.raw = raw != 0;
    if (const int rc = record_files_entry(front, pass, ask, &out)) return rc;
    const WindowsRun& run = out.windows;
    if (n_windows) *n_windows = pass.recs.size();
    if (n_records) *n_records = run.mosaic.size();
    if (n_segments) *n_segments = run.segments.size();
    if (n_changed) *n_changed = run.n_changed;
    if (n_written) *n_written = run.n_written;
    if (bytes_out) *bytes_out = run.fasta.size();
    if (bed_bytes) *bed_bytes = run.bed.size();
    const RowsGift gifts[] = {{(void**)rows, pass.recs.data(), pass.recs.size() * sizeof(spsp_classify_record)},
                              {(void**)hits, pass.hits.data(), pass.hits.size() * sizeof(spsp_classify_hit)},
                              {(void**)first_win, run.first_win.data(), run.first_win.size() * sizeof(uint32_t)},
                              {(void**)segments, run.segments.data(), run.segments.size() * sizeof(spsp_segment_row)},
                              {(void**)mosaic, run.mosaic.data(), run.mosaic.size() * sizeof(spsp_mosaic_row)},
                              {(void**)(raw ? raw_begin : nullptr), run.raw_begin.data(), run.raw_begin.size() * 8},
                              {(void**)(raw ? raw_end : nullptr), run.raw_end.data(), run.raw_end.size() * 8}};
    return give_rows_all(gifts, 7);
}

extern "C" int spsp_classify_files_segments(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                            uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window,
                                            const char* what, spsp_classify_record** rows, spsp_classify_hit** hits, uint64_t* n_windows, uint32_t** first_win,
                                            uint64_t* n_records, spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth,
                                            const char* segments_what, uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out) {
    return spsp_classify_files_raw(ctx, index_paths, n_ref, records_path, top, min_keys, num, den, precision, out_prefix, chatter, rate, window, what, rows, hits, n_windows,
                                   first_win, n_records, segments, n_segments, mosaic, smooth, segments_what, segments_min, gz, n_changed, n_written, bytes_out, 0, nullptr,
                                   nullptr, nullptr);
}

extern "C" int spsp_classify_files_windows(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, uint32_t top, uint32_t min_keys,
                                           uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window,
                                           const char* what, spsp_classify_record** rows, spsp_classify_hit** hits, uint64_t* n_windows, uint32_t** first_win,
                                           uint64_t* n_records, spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic) {
    return spsp_classify_files_segments(ctx, index_paths, n_ref, records_path, top, min_keys, num, den, precision, out_prefix, chatter, rate, window, what, rows, hits,
                                        n_windows, first_win, n_records, segments, n_segments, mosaic, 0, nullptr, 1, 1, nullptr, nullptr, nullptr);
}

extern "C" int spsp_classify_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    ctx->cf_clock.hand_out(ms);
    return SPSP_OK;
}
