// Accumulation on the GPU: how the union (pan) and the intersection (core) of a collection move as its sketches are added one by
// one, over many orders (not in the reference, whose end product is the two n x n matrices).
//
// Keys and notation are the prevalence pass's (spsp_prevalence.hip): sketches 0 .. n-1 back to back, each sorted by (minimizer,
// kmer_hi, kmer_lo); every sketch takes part.  An order is a permutation pi of the sketches; rank(s) = the place of sketch s in it.
// Per distinct key x with holder set H(x):  first(x) = min rank(H(x)),  mex(x) = the least rank not in rank(H(x)), and
//   pan(j)  = #{x : first(x) < j}      core(j) = #{x : mex(x) >= j}        j = 1 .. n
// so an order is two histograms, F[r] = #{x : first = r} and M[r] = #{x : mex = r}, and the host's prefix sums over them.
//
// Built once per call, whatever the number of orders (key_major_build: the classification's index is the same form, spsp_classify.hip):
//   table fill    prevalence's own (prevalence_fill_table, claim = true): holders[e] = h of entry e, bit 31 on the one entry per
//                 distinct key that claimed the key's slot
//   k_ac_prep     a lane per entry: the two scan inputs -- claimer ? 1 : 0 and claimer ? h : 0
//   two scans     launch_scan_u32: the first numbers the distinct keys in entry order, the second gives every claimer the start of
//                 its key's list; the lists together hold exactly the entries, so every size is known without a wait
//   k_ac_scatter  a lane per entry: the probe of k_pv_read, but for the slot; the slot's counter half, which the fill left at h,
//                 is the key's cursor -- one atomic add of -1 hands out the places h-1 .. 0 of the list --, and the entry's sketch
//                 number goes there as 16 bits.  A claimer also writes its key's record: the list's start.  The key-major form is
//                 a CSR over the distinct keys: key_start[0 .. D], the D-th the end; h is the difference of two neighbours, so a
//                 record is ONE word and the claimers need no separate compaction pass.  The order inside a list is a race and
//                 nothing below depends on it (min and mex are functions of the set).  The claimer of a key with more holders
//                 than the cut also appends the key's number to the queue of long lists (one counter, a few thousand adds).
// Per group of G orders, one launch:
//   k_ac_pass<G>  the G rank tables (2 n bytes each) in LDS.  First the short lists: a wave takes 64 consecutive keys, a lane walks
//                 its own list -- consecutive keys' lists are consecutive in memory.  Then the queue of long lists, dealt over
//                 all waves of the grid, one list after another by the whole wave: the claimers of a species' shared keys sit in
//                 the first few sketches, so the long lists of a collection are neighbours in key order and a wave that met them
//                 in its own chunk would meet hundreds (measured: DESIGN 6o).  A list is read ONCE for the G minima.  mex only
//                 where the minimum is 0 (the keys of the order's first sketch): a 64-bit mask for a lane's list, an LDS bitmap of
//                 kAcBitmapBits ranks per pass for the wave's.  F goes through LDS bins over a window of ranks per blockIdx.y and
//                 is flushed once per workgroup with 64-bit adds; M is reached by one sketch's keys per order only and goes to
//                 memory straight, one add per wave and bin from the short lists, one per long list.
// The host waits once, at the end, takes the prefix sums and folds the orders into the rows.  No workgroup waits for another.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kAcThreads = 256;                       // k_ac_prep, k_ac_scatter: 4 waves
constexpr uint32_t kAcWaves = kAcPassThreads / 64;
constexpr uint32_t kAcMapWords = kAcBitmapBits / 32;
enum { kAcwBad = 0, kAcwWrapped = 1, kAcwLong = 2, kAcWords = 4 };   // words in front of the work area: the fill's two flags as it numbers them, the long lists queued

__global__ __launch_bounds__(kAcThreads) void k_ac_prep(const uint32_t* __restrict__ holders, uint32_t n_entries, uint32_t* __restrict__ is_key,
                                                        uint32_t* __restrict__ key_len) {
    const uint64_t i = (uint64_t)blockIdx.x * kAcThreads + threadIdx.x;
    if (i >= n_entries) return;
    const uint32_t v = holders[i], c = v >> 31;
    is_key[i] = c;
    key_len[i] = c ? (v & 0x7fffffffu) : 0u;
}

// holders, key_no, start: indexed by entry number less `first`, as the lists' places are; tbl's slot words name entries as they are
template <bool HAS_HI>
__global__ __launch_bounds__(kAcThreads) void k_ac_scatter(SortedKeys K, const uint64_t* __restrict__ off, uint32_t n, unsigned long long* __restrict__ tbl,
                                                           uint32_t log2cap, const uint32_t* __restrict__ holders, const uint32_t* __restrict__ key_no,
                                                           const uint32_t* __restrict__ start, uint32_t n_entries, uint32_t cut,
                                                           uint32_t* __restrict__ key_start, uint16_t* __restrict__ list, uint32_t* __restrict__ long_keys,
                                                           uint32_t* __restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * kAcThreads + threadIdx.x;
    if (i >= n_entries) return;
    const uint64_t first = off[0], e = first + i;
    if (i == 0) key_start[key_no[n_entries]] = start[n_entries];   // the end of the last list (key_no[n_entries] = D <= n_entries)
    const uint32_t held = holders[i];
    if (held >> 31) {                                      // the key's claimer: its record, and a place in the queue of long lists
        key_start[key_no[i]] = start[i];
        if ((held & 0x7fffffffu) > cut) {
            const uint32_t q = atomicAdd(words + kAcwLong, 1u);
            if (q < n_entries) long_keys[q] = key_no[i];   // (always: a claimer per key, and no more keys than entries)
        }
    }
    const uint32_t mn = K.mn[e];
    const uint64_t lo = K.lo[e], hi = HAS_HI ? K.hi[e] : 0ull;
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t pos = pv_home<HAS_HI>(mn, hi, lo, log2cap);
    for (uint64_t probes = 0;; ++probes) {
        const unsigned long long cur = tbl[pos];
        // (never: the fill gave every entry's key a slot in front of the first free one.  Whatever a caller's arrays hold, no lane goes round)
        if ((uint32_t)cur == 0u || probes > mask) { atomicOr(words + kAcwWrapped, 1u); return; }
        if (pv_same<HAS_HI>(K, (uint64_t)((uint32_t)cur - 1u), mn, hi, lo)) break;
        pos = (pos + 1ull) & mask;
    }
    // the slot's counter is the key's cursor: h on entry, one less per holder, in whatever order the holders arrive
    const unsigned long long was = atomicAdd(&tbl[pos], 0xffffffff00000000ull);
    const uint64_t c = (uint64_t)((uint32_t)was - 1u) - first, r = was >> 32;
    const uint64_t at = c < n_entries ? (uint64_t)start[c] + r - 1ull : ~0ull;
    if (r == 0 || at >= n_entries) { atomicOr(words + kAcwWrapped, 2u); return; }   // (never: the counters add up to the entries)
    list[at] = (uint16_t)sorted_sketch_of(off, 0, n, e);
}

// grid.x = shares of the keys (waves stride over chunks of 64), grid.y = window of `window` ranks of F; LDS: G rank tables of n_pad
// 16-bit words | G x window bins | a bitmap per wave.  ranks, F, M: the group's G rows.  mex is taken by window 0's workgroups alone
template <uint32_t G>
__global__ __launch_bounds__(kAcPassThreads) void k_ac_pass(const uint32_t* __restrict__ key_start, const uint32_t* __restrict__ n_keys_p,
                                                            const uint16_t* __restrict__ list, const uint16_t* __restrict__ ranks, uint32_t n,
                                                            uint32_t n_pad, uint32_t window, uint32_t cut, const uint32_t* __restrict__ long_keys,
                                                            const uint32_t* __restrict__ n_long_p, unsigned long long* __restrict__ F,
                                                            unsigned long long* __restrict__ M) {
    extern __shared__ uint32_t s_mem[];
    const uint16_t* s_rank = reinterpret_cast<const uint16_t*>(s_mem);
    uint32_t* s_bin = s_mem + (size_t)G * (n_pad / 2);
    uint32_t* s_map = s_bin + (size_t)G * window;
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t win_first = blockIdx.y * window;
    const bool with_mex = blockIdx.y == 0;
    for (uint32_t w = threadIdx.x; w < G * (n_pad / 2); w += kAcPassThreads) s_mem[w] = reinterpret_cast<const uint32_t*>(ranks)[w];
    for (uint32_t b = threadIdx.x; b < G * window; b += kAcPassThreads) s_bin[b] = 0u;
    __syncthreads();
    const uint32_t n_keys = *n_keys_p;
    uint32_t* bm = s_map + wid * kAcMapWords;
    for (uint64_t base = ((uint64_t)blockIdx.x * kAcWaves + wid) * 64ull; base < n_keys; base += (uint64_t)gridDim.x * kAcWaves * 64ull) {   // (uniform per wave)
        const uint64_t key = base + lane;
        const bool valid = key < n_keys;
        const uint32_t s = valid ? key_start[key] : 0u, e = valid ? key_start[key + 1] : 0u;
        const uint32_t len = e - s;
        uint32_t fr[G], mx[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) { fr[g] = 0xffffffffu; mx[g] = 0u; }
        if (valid && len <= cut) {                         // the lane's own list
            for (uint32_t i = s; i < e; ++i) {
                const uint32_t sk = list[i];
#pragma unroll
                for (uint32_t g = 0; g < G; ++g) fr[g] = min(fr[g], (uint32_t)s_rank[g * n_pad + sk]);
            }
            if (with_mex) {
#pragma unroll
                for (uint32_t g = 0; g < G; ++g) {
                    if (fr[g] != 0u) continue;
                    unsigned long long seen = 0ull;        // (len <= cut <= 64 ranks: the least one missing is 64 at the most)
                    for (uint32_t i = s; i < e; ++i) {
                        const uint32_t r = s_rank[g * n_pad + list[i]];
                        if (r < 64u) seen |= 1ull << r;
                    }
                    mx[g] = ~seen ? (uint32_t)__ffsll((long long)~seen) - 1u : 64u;
                }
            }
        }
        // F: LDS bins of this window; a wave whose keys all come first at one rank adds once
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t b = fr[g] - win_first;          // (a rank below the window wraps beyond it)
            const bool in = valid && len <= cut && b < window && fr[g] < n;
            const unsigned long long word = __ballot(in);
            if (word != 0ull) {
                const int leader = __ffsll((long long)word) - 1;
                const uint32_t b0 = __shfl(b, leader);
                if (__ballot(in && b != b0) == 0ull) {
                    if ((int)lane == leader) atomicAdd(&s_bin[g * window + b0], (uint32_t)__popcll(word));
                } else if (in) atomicAdd(&s_bin[g * window + b], 1u);
            }
            if (!with_mex) continue;
            // M: only the keys of the order's first sketch come here; one add per wave and bin (one species: one add per wave)
            unsigned long long left = __ballot(valid && len <= cut && fr[g] == 0u && mx[g] >= 1u && mx[g] <= n);
            while (left) {
                const int leader = __ffsll((long long)left) - 1;
                const uint32_t r0 = __shfl(mx[g], leader);
                const unsigned long long same = __ballot(mx[g] == r0) & left;
                if ((int)lane == leader) atomicAdd(&M[(size_t)g * (n + 1u) + r0], (unsigned long long)__popcll(same));
                left &= ~same;
            }
        }
    }
    // the long lists, whichever chunk their keys sit in: one after another by whole waves, dealt over the grid
    const uint32_t n_long = *n_long_p;
    for (uint64_t q = (uint64_t)blockIdx.x * kAcWaves + wid; q < n_long; q += (uint64_t)gridDim.x * kAcWaves) {   // (uniform per wave)
        const uint32_t key = long_keys[q];
        if (key >= n_keys) continue;                       // (never: the scatter numbered them)
        const uint32_t ls = key_start[key], le = key_start[key + 1];
        uint32_t m[G];
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) m[g] = 0xffffffffu;
        for (uint64_t i = (uint64_t)ls + lane; i < le; i += 64ull) {
            const uint32_t sk = list[i];
#pragma unroll
            for (uint32_t g = 0; g < G; ++g) m[g] = min(m[g], (uint32_t)s_rank[g * n_pad + sk]);
        }
#pragma unroll
        for (uint32_t g = 0; g < G; ++g) {
            m[g] = wave_min(m[g]);
            const uint32_t b = m[g] - win_first;           // (a rank below the window wraps beyond it)
            if (lane == 0u && b < window && m[g] < n) atomicAdd(&s_bin[g * window + b], 1u);
            if (!with_mex || m[g] != 0u) continue;         // (uniform: the wave's minimum)
            // mark the ranks of [low, low + kAcBitmapBits) and take the first one missing; all there: the next stretch.  Ranks are
            // below n, so the stretch that holds n -- the last one -- has a zero bit whatever the list holds
            uint32_t mex = n;
            for (uint32_t low = 0; low <= n; low += kAcBitmapBits) {
                for (uint32_t w = lane; w < kAcMapWords; w += 64u) bm[w] = 0u;
                wave_lds_sync();
                for (uint64_t i = (uint64_t)ls + lane; i < le; i += 64ull) {
                    const uint32_t r = (uint32_t)s_rank[g * n_pad + list[i]] - low;   // (a rank below the stretch wraps beyond it)
                    if (r < kAcBitmapBits) atomicOr(&bm[r >> 5], 1u << (r & 31u));
                }
                wave_lds_sync();
                uint32_t cand = 0xffffffffu;
                for (uint32_t w = lane; w < kAcMapWords; w += 64u) {
                    const uint32_t free_bits = ~bm[w];
                    if (free_bits != 0u && cand == 0xffffffffu) cand = w * 32u + (uint32_t)__ffs((int)free_bits) - 1u;
                }
                cand = wave_min(cand);
                wave_lds_sync();                            // (the words are read: the next stretch may clear them)
                if (cand != 0xffffffffu) { mex = low + cand; break; }
            }
            if (lane == 0u && mex >= 1u && mex <= n) atomicAdd(&M[(size_t)g * (n + 1u) + mex], 1ull);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < G * window; b += kAcPassThreads) {
        const uint32_t c = s_bin[b], g = b / window, r = win_first + b % window;
        if (c != 0u && r < n) atomicAdd(&F[(size_t)g * n + r], (unsigned long long)c);
    }
}

template <uint32_t G>
int ac_launch_pass(spsp_ctx* ctx, dim3 grid, size_t lds, const uint32_t* key_start, const uint32_t* n_keys_p, const uint16_t* list, const uint16_t* ranks,
                   uint32_t n, uint32_t n_pad, uint32_t window, uint32_t cut, const uint32_t* long_keys, const uint32_t* n_long_p, unsigned long long* F,
                   unsigned long long* M) {
    if (const int rc = lds_opt_in(ctx, &k_ac_pass<G>, kAcLdsBytes)) return rc;
    hipLaunchKernelGGL(k_ac_pass<G>, grid, dim3(kAcPassThreads), lds, ctx->stream, key_start, n_keys_p, list, ranks, n, n_pad, window, cut, long_keys, n_long_p, F, M);
    return SPSP_OK;
}

}  // namespace

// (spsp_internal.h) the key-major form of the sketches 0 .. n-1: the table fill with claimers, k_ac_prep, the two scans, k_ac_scatter
int key_major_build(spsp_ctx* ctx, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n,
                    uint32_t cut, KeyMajor* out) {
    int rc;
    const uint64_t first = h_sk_off[0];
    const uint32_t E = (uint32_t)(h_sk_off[n] - h_sk_off[0]);
    // work area: flag words | is_key [E] | key_len [E] | key_no [E + 1] | start [E + 1]
    const size_t words_bytes = 64, arr = ((size_t)E + 2) * 4;
    if ((rc = ctx->ac_work.reserve(words_bytes + 4 * arr)) || (rc = ctx->ac_keys.reserve(((size_t)E + 1) * 4)) || (rc = ctx->ac_list.reserve((size_t)E * 2 + 64))) return rc;
    uint32_t* d_words = ctx->ac_work.as<uint32_t>();
    uint32_t* d_is_key = d_words + words_bytes / 4;
    uint32_t* d_key_len = d_is_key + arr / 4;
    uint32_t* d_key_no = d_key_len + arr / 4;
    uint32_t* d_start = d_key_no + arr / 4;
    uint32_t* d_key_start = ctx->ac_keys.as<uint32_t>();
    uint16_t* d_list = ctx->ac_list.as<uint16_t>();
    SPSP_HIP(hipMemsetAsync(d_words, 0, kAcWords * 4, ctx->stream));
    SPSP_HIP(hipMemsetAsync(d_list, 0, (size_t)E * 2, ctx->stream));   // (whatever the scatter leaves out, a list names sketches below n)
    if ((rc = prevalence_fill_table(ctx, has_hi, d_mn, d_lo, d_hi, h_sk_off, n, 0, true, d_words))) return rc;
    const uint64_t* d_off = ctx->pv_off.as<uint64_t>();
    unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
    const uint32_t* d_hold = ctx->pv_hold.as<uint32_t>() + first;
    const SortedKeys K{d_mn, d_lo, d_hi};
    uint32_t* d_long = d_is_key;                           // the queue of long lists: the first scan's input, which is spent by then
    const uint32_t gx = (uint32_t)(((uint64_t)E + kAcThreads - 1) / kAcThreads);
    hipLaunchKernelGGL(k_ac_prep, dim3(gx), dim3(kAcThreads), 0, ctx->stream, d_hold, E, d_is_key, d_key_len);
    SPSP_HIP(hipGetLastError());
    // (the totals stay on the device, in the scans' out[E]: nothing of them comes to the host)
    if ((rc = launch_scan_u32(ctx, d_is_key, d_key_no, E, nullptr)) || (rc = launch_scan_u32(ctx, d_key_len, d_start, E, nullptr))) return rc;
    if (has_hi) hipLaunchKernelGGL(k_ac_scatter<true>, dim3(gx), dim3(kAcThreads), 0, ctx->stream, K, d_off, n, d_tbl, ctx->pv_log2cap, d_hold,
                                   (const uint32_t*)d_key_no, (const uint32_t*)d_start, E, cut, d_key_start, d_list, d_long, d_words);
    else hipLaunchKernelGGL(k_ac_scatter<false>, dim3(gx), dim3(kAcThreads), 0, ctx->stream, K, d_off, n, d_tbl, ctx->pv_log2cap, d_hold,
                            (const uint32_t*)d_key_no, (const uint32_t*)d_start, E, cut, d_key_start, d_list, d_long, d_words);
    SPSP_HIP(hipGetLastError());
    *out = KeyMajor{d_words, d_key_no, d_key_start, d_list, d_long, E};
    return SPSP_OK;
}

int accumulation_check_args(uint32_t n, uint32_t n_orders) {
    if (n == 0 || n > 65535) { set_error("accumulation takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_orders == 0 || n_orders > 1024) { set_error("accumulation takes 1 .. 1024 orders (%u)", n_orders); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

int accumulation_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                             uint32_t n, const uint32_t* orders, uint32_t n_orders, spsp_accumulation_row* rows, uint64_t* pan, uint64_t* core) {
    int rc;
    if (n >= 1 && n <= 65535) memset(rows, 0, (size_t)n * sizeof(spsp_accumulation_row));
    if ((rc = accumulation_check_args(n, n_orders))) return rc;
    const size_t curve_words = (size_t)n_orders * n;
    if (pan) memset(pan, 0, curve_words * 8);
    if (core) memset(core, 0, curve_words * 8);
    KeysShape shape;
    if ((rc = sorted_keys_front(ctx, "accumulation reads", k, d_mn, d_lo, d_hi, h_sk_off, n, &shape))) return rc;
    const bool has_hi = shape.has_hi;
    const uint64_t all_keys = shape.all_keys;
    uint32_t group = 0, window = 0;
    if ((rc = spsp_accumulation_plan_host(n, &group, &window, nullptr, nullptr))) return rc;
    // the orders as rank tables (the inverse permutations), the last group filled up with copies of the last order
    const uint32_t n_pad = (n + 1u) & ~1u, n_groups = (n_orders + group - 1) / group, p_pad = n_groups * group;
    std::vector<uint16_t> rank((size_t)p_pad * n_pad, 0);
    {
        std::vector<uint8_t> seen(n);
        for (uint32_t p = 0; p < n_orders; ++p) {
            std::fill(seen.begin(), seen.end(), 0);
            const uint32_t* o = orders + (size_t)p * n;
            uint16_t* r = rank.data() + (size_t)p * n_pad;
            for (uint32_t j = 0; j < n; ++j) {
                if (o[j] >= n || seen[o[j]]) {
                    set_error("order %u is not a permutation of 0 .. %u: position %u holds %u%s", p, n - 1, j, o[j], o[j] < n ? " again" : "");
                    return SPSP_ERR_ARG;
                }
                seen[o[j]] = 1;
                r[o[j]] = (uint16_t)j;
            }
        }
        for (uint32_t p = n_orders; p < p_pad; ++p) memcpy(rank.data() + (size_t)p * n_pad, rank.data() + (size_t)(n_orders - 1) * n_pad, (size_t)n_pad * 2);
    }
    if (all_keys == 0) return SPSP_OK;                     // (no key anywhere: every curve is 0)
    const uint32_t E = (uint32_t)all_keys;
    const size_t f_words = (size_t)p_pad * n, m_words = (size_t)p_pad * (n + 1u);
    if ((rc = ctx->ac_rank.reserve(rank.size() * 2)) || (rc = ctx->ac_hist.reserve((f_words + m_words) * 8))) return rc;
    uint16_t* d_rank = ctx->ac_rank.as<uint16_t>();
    unsigned long long* d_F = ctx->ac_hist.as<unsigned long long>();
    unsigned long long* d_M = d_F + f_words;
    SPSP_HIP(hipMemsetAsync(d_F, 0, (f_words + m_words) * 8, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(d_rank, rank.data(), rank.size() * 2, hipMemcpyHostToDevice, ctx->stream));   // (rank: alive until the wait)
    uint32_t cut = kAcCut;
    if (const char* dbg = getenv("SPSP_DEBUG_ACCUMULATION_CUT")) {   // (analysis: where the lane's walk ends and the wave's begins, 0 .. 64)
        const long v = atol(dbg);
        if (v >= 0 && v <= 64) cut = (uint32_t)v;
    }
    KeyMajor km;
    if ((rc = key_major_build(ctx, has_hi, d_mn, d_lo, d_hi, h_sk_off, n, cut, &km))) return rc;
    uint32_t* d_words = km.words;
    const uint32_t* d_key_no = km.key_no;
    const uint32_t* d_key_start = km.key_start;
    const uint16_t* d_list = km.list;
    const uint32_t* d_long = km.long_keys;
    // the passes: one launch per group of orders.  A workgroup per CU and as many as the LDS leaves room for, never more than the
    // keys can feed (there are E of them at the most: the number itself stays on the device)
    const size_t lds = (size_t)group * n_pad * 2 + (size_t)group * window * 4 + (size_t)kAcWaves * kAcMapWords * 4;
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(2048 / kAcPassThreads, kAcLdsBytes / lds));
    const uint64_t chunks = ((uint64_t)E + 64ull * kAcWaves - 1) / (64ull * kAcWaves);
    const dim3 grid((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunks, (uint64_t)std::max(ctx->n_cu, 1) * per_cu)), (n + window - 1) / window);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
        const uint16_t* r = d_rank + (size_t)gi * group * n_pad;
        unsigned long long* Fg = d_F + (size_t)gi * group * n;
        unsigned long long* Mg = d_M + (size_t)gi * group * (n + 1u);
        const uint32_t* d_n_keys = d_key_no + E;
        switch (group) {
            case 8: rc = ac_launch_pass<8>(ctx, grid, lds, d_key_start, d_n_keys, d_list, r, n, n_pad, window, cut, d_long, d_words + kAcwLong, Fg, Mg); break;
            case 4: rc = ac_launch_pass<4>(ctx, grid, lds, d_key_start, d_n_keys, d_list, r, n, n_pad, window, cut, d_long, d_words + kAcwLong, Fg, Mg); break;
            case 2: rc = ac_launch_pass<2>(ctx, grid, lds, d_key_start, d_n_keys, d_list, r, n, n_pad, window, cut, d_long, d_words + kAcwLong, Fg, Mg); break;
            default: rc = ac_launch_pass<1>(ctx, grid, lds, d_key_start, d_n_keys, d_list, r, n, n_pad, window, cut, d_long, d_words + kAcwLong, Fg, Mg); break;
        }
        if (rc) return rc;
    }
    SPSP_HIP(hipGetLastError());
    std::vector<uint64_t> F((size_t)n_orders * n), M((size_t)n_orders * (n + 1u));
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsAcBad, d_words, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(F.data(), d_F, F.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(M.data(), d_M, M.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait
    const uint64_t flags = ctx->h_scalar[kHsAcBad];
    if ((uint32_t)flags) { set_error("sketch keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)"); return SPSP_ERR_ARG; }
    if (flags >> 32) { set_error("accumulation: a key's list could not be placed (the key arrays changed during the call?)"); return SPSP_ERR_ARG; }
    // pan(j) = sum of F[r] over r < j, core(j) = sum of M[r] over r >= j; then the rows over the orders
    std::vector<uint64_t> pan_p(n), core_p(n);
    for (uint32_t p = 0; p < n_orders; ++p) {
        const uint64_t* f = F.data() + (size_t)p * n;
        const uint64_t* m = M.data() + (size_t)p * (n + 1u);
        uint64_t acc = 0;
        for (uint32_t j = 1; j <= n; ++j) { acc += f[j - 1]; pan_p[j - 1] = acc; }
        acc = 0;
        for (uint32_t j = n; j >= 1; --j) { acc += m[j]; core_p[j - 1] = acc; }
        if (pan) memcpy(pan + (size_t)p * n, pan_p.data(), (size_t)n * 8);
        if (core) memcpy(core + (size_t)p * n, core_p.data(), (size_t)n * 8);
        for (uint32_t j = 0; j < n; ++j) {
            spsp_accumulation_row& r = rows[j];
            if (p == 0) {
                r.pan_min = r.pan_max = r.pan_sum = r.pan_first = pan_p[j];
                r.core_min = r.core_max = r.core_sum = r.core_first = core_p[j];
            } else {
                r.pan_min = std::min(r.pan_min, pan_p[j]); r.pan_max = std::max(r.pan_max, pan_p[j]); r.pan_sum += pan_p[j];
                r.core_min = std::min(r.core_min, core_p[j]); r.core_max = std::max(r.core_max, core_p[j]); r.core_sum += core_p[j];
            }
        }
    }
    return SPSP_OK;
}

// spsp_accumulation_files behind its argument checks: the sketches loaded (spsp_host.cpp), decoded (and brought down to the common
// rate), the orders from the seed, the curves, <out_prefix>_accumulation.csv.gz
static int accumulation_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_orders, uint64_t seed, int precision, const char* out_prefix,
                              int chatter, double rate, std::vector<spsp_accumulation_row>* rows) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "accumulation is"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    rows->assign(n, spsp_accumulation_row{});
    std::vector<uint32_t> orders((size_t)n_orders * n);
    const DecodedKeys& keys = run.keys;
    rc = spsp_accumulation_orders_host(n, n_orders, seed, orders.data());
    if (!rc) rc = run.decode();
    if (!rc) rc = accumulation_device_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), n, orders.data(), n_orders, rows->data(), nullptr, nullptr);
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; size_t len = 0;
    if ((rc = spsp_accumulation_csv_host(rows->data(), n, n_orders, precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_accumulation.csv.gz", t1)) || !chatter) return rc;
    const spsp_accumulation_row& last = (*rows)[n - 1];
    printf("%u sketch(es) over %u order(s): %llu distinct keys, %llu of them in every sketch\n", n, n_orders, (unsigned long long)last.pan_first,
           (unsigned long long)last.core_first);
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_accumulation_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi,
                                        const uint64_t* h_sk_off, uint32_t n, const uint32_t* orders, uint32_t n_orders, spsp_accumulation_row* rows,
                                        uint64_t* pan, uint64_t* core) {
    if (!ctx || !h_sk_off || !orders || !rows) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return accumulation_device_impl(ctx, k, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n, orders, n_orders,
                                    rows, pan, core);
}

extern "C" int spsp_accumulation_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_orders, uint64_t seed, int precision,
                                       const char* out_prefix, int chatter, double rate, spsp_accumulation_row** rows) {
    if (rows) *rows = nullptr;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = accumulation_check_args(n, n_orders))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_accumulation_row> got;
    if ((rc = accumulation_files(ctx, paths, n, n_orders, seed, precision, out_prefix, chatter, rate, &got))) return rc;
    return rows ? give_rows(got, rows) : SPSP_OK;
}
