// Taxonomy on the GPU: the records of a sequence file assigned to the lowest common ancestor of their keys (not in the reference,
// whose end product is the two n x n matrices).
//
// The index is the classification's (spsp_classify.hip): the prevalence table names a key's claimer entry, key_no[claimer] the key's
// number x in 0 .. D-1, and list[key_start[x] .. key_start[x + 1]) the 16-bit numbers of its holders.  The tree has T nodes in
// preorder: parent[t] < t, the subtree of t is [t, t + size[t]), anc(a, b) = a <= b < a + size[a]; reference j sits at ref_node[j].
//   node(x)  = lca{ ref_node[j] : K_j holds x }                       (once, when the tree is attached)
//   w(t)     = the record's hit keys with node(x) = t                  path(t) = Sum w over t and its ancestors
//   clade(t) = Sum w over the subtree of t                             W = the t with w(t) > 0 of the largest path;  start = lca(W)
//   the call = the first node on the way from start to the root with clade >= min_keys and clade * den >= num * |Q_r|
// Integers only.  In preorder the lca of a set is the lca of its smallest and its largest member (every node between two members
// of one subtree is in that subtree), so both lcas here are a min, a max and one climb of at most 32 parents.
//
// attach (spsp_taxonomy_index_device):
//   k_tx_key_nodes  a lane per distinct key: min and max of ref_node over its list, lists of more than kTxListCut holders by the
//                   whole wave (coalesced), then the climb.  Bound: 2 bytes per holder and one random 4-byte read of ref_node each.
//   k_tx_entry_nodes  only where the caller asks for node(x) per index entry: the probe of depth's numbering pass.
// per batch (spsp_taxonomy_device), one chain of launches whatever the records are, one host wait at its end:
//   k_cf_probe      classify's, unchanged: kn[e] = the key's number + 1, hit[r] = the record's hit keys (its work is not read)
//   k_rec_route     (spsp_device.h) a lane per record: no hit -> its row is written there (TxEmptyRow); hits <= kTxSmallHits -> the
//                   wave form's queue; else the workgroup form's.
//   k_tx_small      a wave per record: node(x) of its hit keys gathered into the wave's 4 KiB of LDS and sorted there
//                   (wave_sort_lds).  The sorted words ARE the prefix sums: the keys in a range of nodes are the difference of two
//                   lower bounds, so w(t), clade(t) = the range [t, t + size[t]) and every term of path(t) are two binary searches
//                   each, and no (node, w) pairs are made.  A lane per run of equal nodes climbs its path; best, min W, max W and
//                   |W| are wave reductions; the confidence climb is at most 33 uniform steps.
//                   Bound: LDS traffic of the sort, (log2 P)^2 / 2 steps over P <= 1 024 words.
//   k_tx_large      a workgroup per record with one 32-bit counter per node: in LDS while 4 T bytes fit beside the fixed words
//                   (T <= kTxLdsNodes), in a row of device memory per workgroup beyond (added to, cleared and read at L2, past
//                   the CU's L1).  One atomic add per hit key; then a lane per node with w > 0 climbs its path over the
//                   counters, and the clades on the way up are range sums that grow from the range below (every counter is read
//                   once at the most).  Bound: hit keys atomic adds + 2 x 4 T bytes of counters per record.
// No workgroup ever waits for another one.  The wave helpers, the route kernel, the call's front and its device arrays are the
// record passes' common ones: spsp_device.h, spsp_internal.h, DESIGN "What the record passes share".
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kTxWaves = kTxThreads / 64, kTxLargeWaves = kTxLargeThreads / 64;
constexpr uint32_t kTxNone = SPSP_TAXONOMY_NONE;
static_assert(kTxSmallHits * 4 * kTxWaves <= 64 * 1024 && (kTxSmallHits & (kTxSmallHits - 1)) == 0, "the wave form's LDS: a power of two of words per wave");
static_assert((size_t)kTxLdsNodes * 4 + kTxLargeFixedLds <= kAcLdsBytes, "the workgroup form's counters beside its fixed words");
static_assert(kTxLargeFixedLds >= (kTxLargeWaves * 5 + kTxLargeWaves) * 4, "the reductions' words");
static_assert(kTxThreads == kRouteThreads && kTxWaves == kRecordWaves, "the record calls' route and wave-form grids");

// the deepest node that is anc of both lo and hi (lo <= hi < T): the first ancestor of lo whose subtree reaches hi
__device__ __forceinline__ uint32_t tx_lca(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size, uint32_t lo, uint32_t hi) {
    uint32_t a = lo;
    for (uint32_t step = 0; step <= kTxMaxDepth && a != 0u && hi - a >= size[a]; ++step) a = parent[a];   // (the root holds every node)
    return a;
}

// what a lane knows of W so far: the best path it met, and of the nodes with that path the smallest, the largest and their number
struct TxBest { uint32_t best, lo, hi, count; };
__device__ __forceinline__ void tx_meet(TxBest& b, uint32_t path, uint32_t t) {
    if (path > b.best) { b.best = path; b.lo = b.hi = t; b.count = 1u; }
    else if (path == b.best) { b.lo = t < b.lo ? t : b.lo; b.hi = t > b.hi ? t : b.hi; ++b.count; }
}
// ... and the wave's: every lane gets it
__device__ __forceinline__ TxBest tx_best_of_wave(TxBest b) {
    const uint32_t best = wave_max(b.best);
    const bool mine = b.best == best && b.count != 0u;
    TxBest o;
    o.best = best;
    o.lo = wave_min(mine ? b.lo : kTxNone);
    o.hi = wave_max(mine ? b.hi : 0u);
    o.count = wave_sum(mine ? b.count : 0u);
    return o;
}

// node(x) of every distinct key x < D = key_no[n_index]: the lca of its holders' nodes
__global__ __launch_bounds__(kTxThreads) void k_tx_key_nodes(const uint32_t* __restrict__ key_no, uint32_t n_index, const uint32_t* __restrict__ key_start,
                                                             const uint16_t* __restrict__ list, uint32_t R, const uint32_t* __restrict__ ref_node,
                                                             const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size, uint32_t T,
                                                             uint32_t* __restrict__ key_node) {
    const uint32_t D = min(key_no[n_index], n_index);
    const uint64_t x = (uint64_t)blockIdx.x * kTxThreads + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = x < D;
    const uint32_t ls = valid ? key_start[x] : 0u, len = valid ? key_start[x + 1u] - ls : 0u;
    uint32_t lo = kTxNone, hi = 0u;
    if (len <= kTxListCut)
        for (uint32_t j = 0; j < len; ++j) {
            const uint32_t sk = list[ls + j];
            if (sk < R) { const uint32_t t = ref_node[sk]; lo = t < lo ? t : lo; hi = t > hi ? t : hi; }
        }
    wave_long_lists(len > kTxListCut, ls, len, [=, &lo, &hi](int l, uint32_t s0, uint32_t n0) {
        uint32_t a = kTxNone, b = 0u;
        for (uint32_t j = lane; j < n0; j += 64u) {
            const uint32_t sk = list[s0 + j];
            if (sk < R) { const uint32_t t = ref_node[sk]; a = t < a ? t : a; b = t > b ? t : b; }
        }
        a = wave_min(a); b = wave_max(b);
        if ((int)lane == l) { lo = a; hi = b; }
    });
    if (!valid) return;
    key_node[x] = lo < T && hi < T ? tx_lca(parent, size, lo, hi) : 0u;   // (a key always has a holder, and ref_node < T was checked)
}

// node(x) per index entry: the entry's own key looked up as depth's numbering pass does it
template <bool HAS_HI>
__global__ __launch_bounds__(kTxThreads) void k_tx_entry_nodes(SortedKeys K, uint64_t first, uint32_t n_index, const unsigned long long* __restrict__ tbl,
                                                               uint32_t log2cap, const uint32_t* __restrict__ key_no, const uint32_t* __restrict__ key_node,
                                                               uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kTxThreads + threadIdx.x;
    if (i >= n_index) return;
    const uint32_t D = min(key_no[n_index], n_index);
    const uint64_t e = first + i;
    const uint64_t at = pv_find<HAS_HI>(K, first, n_index, tbl, log2cap, K.mn[e], HAS_HI ? K.hi[e] : 0ull, K.lo[e]);
    uint32_t node = kTxNone;
    if (at != ~0ull) {                                     // (always: the table was filled from these entries)
        const uint32_t number = key_no[at];
        if (number < D) node = key_node[number];
    }
    out[i] = node;
}

// a record's eight words: keys, hit_keys, node, start | score, clade, direct, winners
__device__ __forceinline__ void tx_write(uint4* __restrict__ rec, uint32_t r, uint32_t keys, uint32_t hit_keys, uint32_t node, uint32_t start, uint32_t score,
                                         uint32_t clade, uint32_t direct, uint32_t winners) {
    rec[2ull * r] = make_uint4(keys, hit_keys, node, start);
    rec[2ull * r + 1ull] = make_uint4(score, clade, direct, winners);
}

// the row of a record without a hit key, which the route kernel writes
struct TxEmptyRow {
    __device__ void operator()(uint4* __restrict__ rec, uint32_t r, uint32_t keys) const { tx_write(rec, r, keys, 0u, kTxNone, kTxNone, 0u, 0u, 0u, 0u); }
};

// a wave per queued record; kn, and the entries of off, count from the first record key
__global__ __launch_bounds__(kTxThreads) void k_tx_small(const uint64_t* __restrict__ off, const uint32_t* __restrict__ kn_of, const uint32_t* __restrict__ key_node,
                                                         const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size, uint32_t T,
                                                         const uint32_t* __restrict__ q_small, uint32_t* __restrict__ words, uint32_t min_keys, uint32_t num,
                                                         uint32_t den, uint4* __restrict__ rec) {
    __shared__ uint32_t s_all[kTxWaves][kTxSmallHits];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t* s = s_all[wid];
    const uint32_t n_small = words[kRqSmall];
    const uint64_t q0 = off[0];
    for (uint64_t q = (uint64_t)blockIdx.x * kTxWaves + wid; q < n_small; q += (uint64_t)gridDim.x * kTxWaves) {   // (uniform per wave)
        const uint32_t r = q_small[q];
        const uint64_t a = off[r] - q0, z = off[r + 1] - q0;
        const uint32_t keys = (uint32_t)(z - a);
        // the nodes of the record's hit keys, packed
        uint32_t H = 0;
        bool fits = true;
        for (uint64_t base = a; base < z; base += 64ull) {
            const uint64_t i = base + lane;
            const uint32_t kn = i < z ? kn_of[i] : 0u;
            const uint32_t node = kn ? key_node[kn - 1u] : kTxNone;
            const bool has = node < T;
            const unsigned long long b = __ballot(has);
            const uint32_t n = (uint32_t)__popcll(b);
            if (n > kTxSmallHits - H) { fits = false; break; }   // (never: the route sent a record of this many hits elsewhere.  Uniform)
            if (has) s[H + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = node;
            H += n;
        }
        if (!fits || H == 0u) { if (lane == 0u) atomicOr(words + kRqBad, 1u); continue; }
        uint32_t P = 64;
        while (P < H) P <<= 1;
        for (uint32_t i = H + lane; i < P; i += 64u) s[i] = kTxNone;
        wave_sort_lds(s, P, lane);
        // every run of one node t has w(t) > 0: the lane at its last place climbs path(t)
        TxBest mine{0u, kTxNone, 0u, 0u};
        for (uint32_t base = 0; base < H; base += 64u) {
            const uint32_t i = base + lane;
            if (i < H) {
                const uint32_t t = s[i];
                if (i + 1u == H || s[i + 1u] != t) {
                    uint32_t path = i + 1u - lds_lower_bound(s, i, t), at = t;
                    for (uint32_t step = 0; step < kTxMaxDepth && at != 0u; ++step) {
                        at = parent[at];
                        const uint32_t lo = lds_lower_bound(s, H, at);
                        path += lds_lower_bound(s, H, at + 1u) - lo;
                    }
                    tx_meet(mine, path, t);
                }
            }
        }
        const TxBest W = tx_best_of_wave(mine);
        const uint32_t start = tx_lca(parent, size, W.lo, W.hi);
        uint32_t node = kTxNone, clade = 0u, direct = 0u, t = start;
        for (uint32_t step = 0; step <= kTxMaxDepth; ++step) {   // (uniform: every lane walks the same way up)
            const uint32_t lo = lds_lower_bound(s, H, t), c = lds_lower_bound(s, H, t + size[t]) - lo;
            if (passes_threshold(c, keys, min_keys, num, den)) { node = t; clade = c; direct = lds_lower_bound(s, H, t + 1u) - lo; break; }
            if (t == 0u) break;
            t = parent[t];
        }
        wave_lds_sync();                                    // (the words are read: the next record may overwrite them)
        if (lane == 0u) tx_write(rec, r, keys, H, node, start, W.best, clade, direct, W.count);
    }
}

// sums over the workgroup: every lane gets the total.  s8: kTxLargeWaves words nobody else uses between the two barriers inside
__device__ __forceinline__ uint32_t tx_block_sum(uint32_t v, uint32_t* s8, uint32_t lane, uint32_t wid) {
    v = wave_sum(v);
    if (lane == 0u) s8[wid] = v;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kTxLargeWaves; ++w) total += s8[w];
    __syncthreads();
    return total;
}

// a workgroup per queued record.  LDS: [IN_LDS: T_pad counters |] the waves' W words (5 each) | the sums' words.  rows: !IN_LDS, a row
// of T_pad counters per workgroup
template <bool IN_LDS>
__global__ __launch_bounds__(kTxLargeThreads) void k_tx_large(const uint64_t* __restrict__ off, const uint32_t* __restrict__ kn_of,
                                                              const uint32_t* __restrict__ key_node, const uint32_t* __restrict__ parent,
                                                              const uint32_t* __restrict__ size, uint32_t T, uint32_t T_pad, const uint32_t* __restrict__ q_large,
                                                              const uint32_t* __restrict__ words, uint32_t* __restrict__ rows, uint32_t min_keys, uint32_t num,
                                                              uint32_t den, uint4* __restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    uint32_t* cnt = IN_LDS ? s_mem : rows + (size_t)blockIdx.x * T_pad;
    uint32_t* s_w = s_mem + (IN_LDS ? T_pad : 0u);         // wave w: best, lo, hi, count, hits at s_w[5 w ..]
    uint32_t* s8 = s_w + kTxLargeWaves * 5u;
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t n_large = words[kRqLarge];
    const uint64_t q0 = off[0];
    // (the rows in device memory are added to at L2: they are cleared and read there as well, past this CU's L1)
    auto get = [&](uint32_t j) -> uint32_t { return IN_LDS ? cnt[j] : __hip_atomic_load(cnt + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    for (uint64_t q = blockIdx.x; q < n_large; q += gridDim.x) {   // (uniform per workgroup)
        const uint32_t r = q_large[q];
        const uint64_t a = off[r] - q0, z = off[r + 1] - q0;
        const uint32_t keys = (uint32_t)(z - a);
        for (uint32_t j = threadIdx.x; j < T; j += kTxLargeThreads) {
            if (IN_LDS) cnt[j] = 0u;
            else __hip_atomic_store(cnt + j, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        for (uint64_t i = a + threadIdx.x; i < z; i += kTxLargeThreads) {
            const uint32_t kn = kn_of[i];
            if (kn) { const uint32_t t = key_node[kn - 1u]; if (t < T) atomicAdd(&cnt[t], 1u); }
        }
        __syncthreads();
        // a lane per node with w > 0: its path over the counters
        TxBest mine{0u, kTxNone, 0u, 0u};
        uint32_t hits = 0;
        for (uint32_t t = threadIdx.x; t < T; t += kTxLargeThreads) {
            const uint32_t w = get(t);
            if (w == 0u) continue;
            hits += w;
            uint32_t path = w, at = t;
            for (uint32_t step = 0; step < kTxMaxDepth && at != 0u; ++step) { at = parent[at]; path += get(at); }
            tx_meet(mine, path, t);
        }
        const TxBest mw = tx_best_of_wave(mine);
        hits = wave_sum(hits);
        if (lane == 0u) { uint32_t* o = s_w + wid * 5u; o[0] = mw.best; o[1] = mw.lo; o[2] = mw.hi; o[3] = mw.count; o[4] = hits; }
        __syncthreads();
        TxBest W{0u, kTxNone, 0u, 0u};
        uint32_t H = 0;
        for (uint32_t w = 0; w < kTxLargeWaves; ++w) {     // (every lane merges the eight: the same words, the same result)
            const uint32_t* o = s_w + w * 5u;
            H += o[4];
            if (o[3] == 0u || o[0] < W.best) continue;
            if (o[0] > W.best) { W.best = o[0]; W.lo = o[1]; W.hi = o[2]; W.count = o[3]; }
            else { W.lo = o[1] < W.lo ? o[1] : W.lo; W.hi = o[2] > W.hi ? o[2] : W.hi; W.count += o[3]; }
        }
        uint32_t node = kTxNone, start = kTxNone, clade = 0u, direct = 0u;
        if (W.count != 0u) {                               // (uniform.  Always: the route saw hit keys)
            start = tx_lca(parent, size, W.lo, W.hi);
            // the way up: the clade of a node is its child's and the counters of its range on both sides of the child's
            uint32_t t = start, lo = start, hi = start, c = 0u;
            for (uint32_t step = 0; step <= kTxMaxDepth; ++step) {
                const uint32_t n_lo = t, n_hi = t + size[t];
                uint32_t part = 0;
                for (uint32_t j = n_lo + threadIdx.x; j < lo; j += kTxLargeThreads) part += get(j);
                for (uint32_t j = hi + threadIdx.x; j < n_hi; j += kTxLargeThreads) part += get(j);
                c += tx_block_sum(part, s8, lane, wid);
                lo = n_lo; hi = n_hi;
                if (passes_threshold(c, keys, min_keys, num, den)) { node = t; clade = c; direct = get(t); break; }
                if (t == 0u) break;
                t = parent[t];
            }
        }
        if (threadIdx.x == 0u) tx_write(rec, r, keys, H, node, start, W.best, clade, direct, W.count);
        __syncthreads();                                   // (the counters and the waves' words are read: the next record clears them)
    }
}

}  // namespace

int taxonomy_index_impl(spsp_ctx* ctx, const uint32_t* parent, uint32_t T, const uint32_t* ref_node, uint32_t n_ref, const uint32_t** key_nodes_out) {
    int rc;
    if (key_nodes_out) *key_nodes_out = nullptr;
    spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    if (!X.valid) return refuse_no_index("taxonomy");
    if (n_ref != X.n_ref) { set_error("taxonomy: %u references, the index holds %u", n_ref, X.n_ref); return SPSP_ERR_ARG; }
    if ((rc = spsp_taxonomy_check_host(parent, T, ref_node, n_ref))) return rc;
    X.taxonomy = false;
    std::vector<uint32_t> size(T, 1);
    for (uint32_t t = T - 1; t >= 1; --t) size[parent[t]] += size[t];
    const uint32_t E = X.entries, T_pad = (T + 3u) & ~3u;
    if ((rc = ctx->tx_tree.reserve(((size_t)2 * T_pad + n_ref) * 4 + 64)) || (rc = ctx->tx_key_node.reserve((size_t)E * 4 + 64)) ||
        (key_nodes_out && (rc = ctx->tx_entry_node.reserve((size_t)E * 4 + 64)))) return rc;
    uint32_t* d_parent = ctx->tx_tree.as<uint32_t>();
    uint32_t *d_size = d_parent + T_pad, *d_ref = d_size + T_pad;
    SPSP_HIP(hipMemcpyAsync(d_parent, parent, (size_t)T * 4, hipMemcpyHostToDevice, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(d_size, size.data(), (size_t)T * 4, hipMemcpyHostToDevice, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(d_ref, ref_node, (size_t)n_ref * 4, hipMemcpyHostToDevice, ctx->stream));
    if (E) {
        const uint32_t gx = (uint32_t)(((uint64_t)E + kTxThreads - 1) / kTxThreads);   // (D <= E: a grid over the entries covers the keys)
        hipLaunchKernelGGL(k_tx_key_nodes, dim3(gx), dim3(kTxThreads), 0, ctx->stream, X.key_no, E, X.key_start, X.list, n_ref, (const uint32_t*)d_ref,
                           (const uint32_t*)d_parent, (const uint32_t*)d_size, T, ctx->tx_key_node.as<uint32_t>());
        SPSP_HIP(hipGetLastError());
        if (key_nodes_out) {
            const SortedKeys K{X.mn, X.lo, X.hi};
            const unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
            if (X.has_hi) hipLaunchKernelGGL(k_tx_entry_nodes<true>, dim3(gx), dim3(kTxThreads), 0, ctx->stream, K, X.first, E, d_tbl, ctx->pv_log2cap, X.key_no,
                                             (const uint32_t*)ctx->tx_key_node.as<uint32_t>(), ctx->tx_entry_node.as<uint32_t>());
            else hipLaunchKernelGGL(k_tx_entry_nodes<false>, dim3(gx), dim3(kTxThreads), 0, ctx->stream, K, X.first, E, d_tbl, ctx->pv_log2cap, X.key_no,
                                    (const uint32_t*)ctx->tx_key_node.as<uint32_t>(), ctx->tx_entry_node.as<uint32_t>());
            SPSP_HIP(hipGetLastError());
        }
    }
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the attach's wait (the caller's arrays and `size` live until here)
    if (key_nodes_out) *key_nodes_out = ctx->tx_entry_node.as<uint32_t>();
    X.tx_nodes = T;
    X.taxonomy = true;
    return SPSP_OK;
}

int taxonomy_device_impl(spsp_ctx* ctx, const uint32_t* q_mn, const uint64_t* q_lo, const uint64_t* q_hi, const uint64_t* h_rec_off, uint32_t n_rec,
                         uint32_t min_keys, uint32_t num, uint32_t den, spsp_taxonomy_record* records) {
    int rc;
    // (what is zeroed in front of the refusals: everything but the caller's lengths)
    for (uint32_t r = 0; r < n_rec; ++r) { const uint64_t length = records[r].length; records[r] = spsp_taxonomy_record{}; records[r].length = length; }
    uint64_t all_keys = 0;
    if ((rc = taxonomy_check_args(min_keys, num, den)) || (rc = record_call_front(ctx, "taxonomy", true, q_mn, q_lo, q_hi, h_rec_off, n_rec, &all_keys))) return rc;
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    for (uint32_t r = 0; r < n_rec; ++r) {                 // (length is the caller's)
        records[r].keys = (uint32_t)(h_rec_off[r + 1] - h_rec_off[r]);
        records[r].node = records[r].start = kTxNone;
    }
    if (n_rec == 0 || all_keys == 0 || X.entries == 0) return SPSP_OK;   // (no record, no record key or no reference key: no hit)

    const uint32_t T = X.tx_nodes, T_pad = (T + 3u) & ~3u;
    const bool in_lds = T <= kTxLdsNodes;
    const int n_cu = std::max(ctx->n_cu, 1);
    const size_t lds = kTxLargeFixedLds + (in_lds ? (size_t)T_pad * 4 : 0);
    const uint32_t large_per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(2048 / kTxLargeThreads, kAcLdsBytes / lds));
    // (the rows in device memory: as many workgroups as rows fit kTxRowsBytes, one per CU at the most)
    const uint64_t rows_fit = std::max<uint64_t>(1, kTxRowsBytes / ((size_t)T_pad * 4));
    const uint32_t g_large = (uint32_t)std::min<uint64_t>(n_rec, in_lds ? (uint64_t)n_cu * large_per_cu : std::min<uint64_t>((uint64_t)n_cu, rows_fit));
    RecordWork W;
    if ((rc = W.reserve(ctx, n_rec, all_keys, 32)) || (!in_lds && (rc = ctx->cf_rows.reserve((size_t)g_large * T_pad * 4)))) return rc;
    uint32_t* d_rows = in_lds ? nullptr : ctx->cf_rows.as<uint32_t>();
    const uint32_t* d_parent = ctx->tx_tree.as<uint32_t>();
    const uint32_t* d_size = d_parent + T_pad;
    const uint32_t* d_key_node = ctx->tx_key_node.as<uint32_t>();
    RecordClock& clock = ctx->tx_clock;
    if ((rc = W.upload(ctx, h_rec_off)) || (rc = W.clear(ctx)) || (rc = clock.mark(ctx, 0)) ||
        (rc = classify_probe_launch(ctx, q_mn, q_lo, q_hi, W.off, n_rec, all_keys, W.kn, W.work, W.hit)) || (rc = clock.mark(ctx, 1))) return rc;
    hipLaunchKernelGGL((k_rec_route<uint32_t, TxEmptyRow>), dim3(W.g_route), dim3(kRouteThreads), 0, ctx->stream, (const uint64_t*)W.off, n_rec, (const uint32_t*)W.hit,
                       kTxSmallHits, W.words, W.q_small, W.q_large, W.rec, TxEmptyRow{});
    if ((rc = clock.mark(ctx, 2))) return rc;
    hipLaunchKernelGGL(k_tx_small, dim3(W.g_small), dim3(kTxThreads), 0, ctx->stream, (const uint64_t*)W.off, (const uint32_t*)W.kn, d_key_node, d_parent, d_size, T,
                       (const uint32_t*)W.q_small, W.words, min_keys, num, den, W.rec);
    if ((rc = clock.mark(ctx, 3))) return rc;
    if (in_lds) {
        if ((rc = lds_opt_in(ctx, &k_tx_large<true>, kAcLdsBytes))) return rc;
        hipLaunchKernelGGL(k_tx_large<true>, dim3(g_large), dim3(kTxLargeThreads), lds, ctx->stream, (const uint64_t*)W.off, (const uint32_t*)W.kn, d_key_node,
                           d_parent, d_size, T, T_pad, (const uint32_t*)W.q_large, (const uint32_t*)W.words, d_rows, min_keys, num, den, W.rec);
    } else {
        hipLaunchKernelGGL(k_tx_large<false>, dim3(g_large), dim3(kTxLargeThreads), lds, ctx->stream, (const uint64_t*)W.off, (const uint32_t*)W.kn, d_key_node,
                           d_parent, d_size, T, T_pad, (const uint32_t*)W.q_large, (const uint32_t*)W.words, d_rows, min_keys, num, den, W.rec);
    }
    SPSP_HIP(hipGetLastError());
    if ((rc = clock.mark(ctx, 4))) return rc;
    std::vector<uint32_t> got;
    bool fitted = false;
    if ((rc = W.read_back(ctx, &got)) || (rc = W.wait(ctx, clock, &fitted))) return rc;
    if (!fitted) {
        set_error("taxonomy: a record's hit keys did not fit the form it was routed to (the key arrays changed during the call?)");
        for (uint32_t r = 0; r < n_rec; ++r) { const uint64_t length = records[r].length; records[r] = spsp_taxonomy_record{}; records[r].length = length; }
        return SPSP_ERR_ARG;
    }
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint32_t* g = got.data() + (size_t)r * 8;
        spsp_taxonomy_record& o = records[r];
        o.keys = g[0]; o.hit_keys = g[1]; o.node = g[2]; o.start = g[3]; o.score = g[4]; o.clade = g[5]; o.direct = g[6]; o.winners = g[7];
    }
    return SPSP_OK;
}

// taxonomy as a record pass: the tree of the lineage file (the pass owns its four arrays), the rows of all records (windows) on
// the host, a batch's call into its stretch of them
struct TaxonomyPass : RecordPass {
    spsp_ctx* ctx;
    uint32_t n_ref, min_keys, num, den;
    const char* lineages_path;
    std::vector<uint32_t> ref_node;
    uint32_t *parent = nullptr, *depth = nullptr, *size = nullptr, T = 0;
    char* blob = nullptr;
    std::vector<const char*> node_names;
    std::vector<spsp_taxonomy_record> recs;
    explicit TaxonomyPass(const RecordFront& f) : ctx(f.ctx), n_ref(f.n_ref), min_keys(f.min_keys), num(f.num), den(f.den), lineages_path(f.lineages_path) {}
    ~TaxonomyPass() override { spsp_free(parent); spsp_free(depth); spsp_free(size); spsp_free(blob); }
    // the lineage file first: a tree that cannot be read costs no loading
    int prelude(const RecordsAsk& ask) override {
        int rc;
        uint8_t* lin = nullptr; uint64_t n_lin = 0, blob_len = 0;
        if ((rc = spsp_read_file_host(lineages_path, &lin, &n_lin))) return rc;
        ref_node.assign(n_ref, 0);
        const bool cuts = ask.mode == kRmExtract || ask.mode == kRmSplit;
        rc = spsp_taxonomy_lineages_host((const char*)lin, n_lin, n_ref, ref_node.data(), &parent, &depth, cuts ? &size : nullptr, &blob, &blob_len, &T);
        spsp_free(lin);
        if (rc) return rc;
        // (the word's node against the tree: still before any sketch is read)
        if (ask.mode == kRmExtract && (rc = spsp_extract_word_check_host(ask.what, 1, T))) return rc;
        if ((rc = segments_ask_check(ask, 1, T + 1))) return rc;   // (likewise <b> of a windowed run's selection: the bins are the nodes and "unclassified")
        node_names.resize(T);
        for (uint64_t at = 0, t = 0; t < T; ++t) { node_names[t] = blob + at; at += strlen(blob + at) + 1; }
        return SPSP_OK;
    }
    int on_index() override { return taxonomy_index_impl(ctx, parent, T, ref_node.data(), n_ref, nullptr); }
    int on_records(uint32_t n_rec, const uint64_t* rec_off) override {
        recs.assign(n_rec, spsp_taxonomy_record{});
        for (uint32_t r = 0; r < n_rec; ++r) recs[r].length = rec_off[r + 1] - rec_off[r];
        return SPSP_OK;
    }
    int on_batch(const RecordBatch& B) override {
        return taxonomy_device_impl(ctx, B.mn, B.lo, B.hi, B.key_off, B.n_records, min_keys, num, den, recs.data() + B.first_record);
    }
    int keep_flags(const char* what, uint32_t n, uint8_t* keep) override { return spsp_extract_flags_taxonomy_host(what, recs.data(), n, size, T, keep); }
    int bins(const char* what, uint32_t n, uint32_t* bin, uint32_t* n_bins) override {
        return spsp_split_bins_taxonomy_host(what, recs.data(), n, parent, depth, T, bin, n_bins);
    }
    void window_addends(size_t w, uint32_t* keys, uint32_t* hit_keys, uint32_t* support) override {
        *keys = recs[w].keys; *hit_keys = recs[w].hit_keys;
        *support = recs[w].node != kTxNone ? recs[w].clade : 0u;
    }
    const char* const* bin_names() override { return node_names.data(); }   // (the names the report prints: the nodes')
    const char* last_name() override { return "unclassified"; }
    size_t n_rows() override { return recs.size(); }
    int write_rows(FilesRun&, const RecordsAsk& ask, const std::vector<std::string>& names, double t1) override {
        int rc;
        std::vector<const char*> name_ptr(names.size());
        for (size_t r = 0; r < names.size(); ++r) name_ptr[r] = names[r].c_str();
        char *text = nullptr, *report = nullptr; uint64_t len = 0, report_len = 0;
        // (both texts before either file: nothing is written where a row is refused)
        if ((rc = spsp_taxonomy_csv_host(recs.data(), recs.size(), name_ptr.data(), parent, T, node_names.data(), ask.precision, &text, &len))) return rc;
        if ((rc = spsp_taxonomy_report_csv_host(recs.data(), recs.size(), parent, T, node_names.data(), ref_node.data(), n_ref, &report, &report_len))) {
            spsp_free(text);
            return rc;
        }
        if ((rc = write_csv_gz(ctx, text, len, ask.out_prefix, "_taxonomy.csv.gz", t1))) { spsp_free(report); return rc; }   // (the text is taken over)
        return write_csv_gz(ctx, report, report_len, ask.out_prefix, "_taxonomy_report.csv.gz", now_s());
    }
    void say_rows(FilesRun&, const RecordsAsk& ask) override {
        uint64_t called = 0, at_root = 0;
        for (const spsp_taxonomy_record& r : recs) { called += r.node != kTxNone; at_root += r.node == 0u; }
        printf(ask.mates_path ? "%zu pair(s) against %u reference(s) at %u node(s): %llu classified, %.3g of them at depth 0\n"
                              : "%zu record(s) against %u reference(s) at %u node(s): %llu classified, %.3g of them at depth 0\n", recs.size(), n_ref, T, (unsigned long long)called,
               called ? (double)at_root / (double)called : 0.0);
    }
};

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_taxonomy_index_device(spsp_ctx* ctx, const uint32_t* parent, uint32_t n_nodes, const uint32_t* ref_node, uint32_t n_ref,
                                          const void** key_nodes_out) {
    if (key_nodes_out) *key_nodes_out = nullptr;
    if (!ctx || !parent || !ref_node) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    const uint32_t* out = nullptr;
    const int rc = taxonomy_index_impl(ctx, parent, n_nodes, ref_node, n_ref, key_nodes_out ? &out : nullptr);
    if (key_nodes_out) *key_nodes_out = out;
    return rc;
}

extern "C" int spsp_taxonomy_device(spsp_ctx* ctx, const void* d_q_minimizer, const void* d_q_kmer_lo, const void* d_q_kmer_hi, const uint64_t* h_rec_off,
                                    uint32_t n_records, uint32_t min_keys, uint32_t num, uint32_t den, spsp_taxonomy_record* records) {
    if (!ctx || !h_rec_off || (n_records && !records)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return taxonomy_device_impl(ctx, (const uint32_t*)d_q_minimizer, (const uint64_t*)d_q_kmer_lo, (const uint64_t*)d_q_kmer_hi, h_rec_off, n_records, min_keys,
                                num, den, records);
}

// spsp_taxonomy_files, _extract, _paired and _split behind the filling of their ask: the outputs cleared, the front and the
// driver, the rows handed out
static int taxonomy_files_entry(const RecordFront& front, const RecordsAsk& ask, spsp_taxonomy_record** records, uint64_t* n_records, uint64_t* n_kept,
                                uint64_t* bytes_out) {
    if (records) *records = nullptr;
    if (n_records) *n_records = 0;
    if (n_kept) *n_kept = 0;
    if (bytes_out) *bytes_out = 0;
    TaxonomyPass pass(front);
    RecordsOut out;
    if (const int rc = record_files_entry(front, pass, ask, &out)) return rc;
    if (n_kept) *n_kept = out.n_kept(ask);
    if (bytes_out) *bytes_out = out.bytes_out();
    if (n_records) *n_records = pass.recs.size();
    const RowsGift gift{(void**)records, pass.recs.data(), pass.recs.size() * sizeof(spsp_taxonomy_record)};
    return give_rows_all(&gift, 1);
}

extern "C" int spsp_taxonomy_files_raw(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                            uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                            uint64_t window, const char* what, spsp_taxonomy_record** rows, uint64_t* n_windows, uint32_t** first_win,
                                            uint64_t* n_records, spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth,
                                            const char* segments_what, uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out, int raw,
                                       uint64_t** raw_begin, uint64_t** raw_end, uint64_t* bed_bytes) {
    if (rows) *rows = nullptr;
    if (first_win) *first_win = nullptr;
    if (segments) *segments = nullptr;
    if (mosaic) *mosaic = nullptr;
    if (raw_begin) *raw_begin = nullptr;
    if (raw_end) *raw_end = nullptr;
    for (uint64_t* n : {n_windows, n_records, n_segments, n_changed, n_written, bytes_out, bed_bytes}) if (n) *n = 0;
    const RecordFront front{ctx, index_paths, lineages_path, true, false, n_ref, 0, min_keys, num, den};
    TaxonomyPass pass(front);
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
    const RowsGift gifts[] = {{(void**)rows, pass.recs.data(), pass.recs.size() * sizeof(spsp_taxonomy_record)},
                              {(void**)first_win, run.first_win.data(), run.first_win.size() * sizeof(uint32_t)},
                              {(void**)segments, run.segments.data(), run.segments.size() * sizeof(spsp_segment_row)},
                              {(void**)mosaic, run.mosaic.data(), run.mosaic.size() * sizeof(spsp_mosaic_row)},
                              {(void**)(raw ? raw_begin : nullptr), run.raw_begin.data(), run.raw_begin.size() * 8},
                              {(void**)(raw ? raw_end : nullptr), run.raw_end.data(), run.raw_end.size() * 8}};
    return give_rows_all(gifts, 6);
}

extern "C" int spsp_taxonomy_files_segments(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                            uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                            uint64_t window, const char* what, spsp_taxonomy_record** rows, uint64_t* n_windows, uint32_t** first_win,
                                            uint64_t* n_records, spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic, uint32_t smooth,
                                            const char* segments_what, uint64_t segments_min, int gz, uint64_t* n_changed, uint64_t* n_written, uint64_t* bytes_out) {
    return spsp_taxonomy_files_raw(ctx, index_paths, n_ref, records_path, lineages_path, min_keys, num, den, precision, out_prefix, chatter, rate, window, what, rows,
                                   n_windows, first_win, n_records, segments, n_segments, mosaic, smooth, segments_what, segments_min, gz, n_changed, n_written, bytes_out, 0,
                                   nullptr, nullptr, nullptr);
}

extern "C" int spsp_taxonomy_files_windows(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                           uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate, uint64_t window,
                                           const char* what, spsp_taxonomy_record** rows, uint64_t* n_windows, uint32_t** first_win, uint64_t* n_records,
                                           spsp_segment_row** segments, uint64_t* n_segments, spsp_mosaic_row** mosaic) {
    return spsp_taxonomy_files_segments(ctx, index_paths, n_ref, records_path, lineages_path, min_keys, num, den, precision, out_prefix, chatter, rate, window, what, rows,
                                        n_windows, first_win, n_records, segments, n_segments, mosaic, 0, nullptr, 1, 1, nullptr, nullptr, nullptr);
}

extern "C" int spsp_taxonomy_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                   uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                   spsp_taxonomy_record** records, uint64_t* n_records) {
    return taxonomy_files_entry({ctx, index_paths, lineages_path, true, false, n_ref, 0, min_keys, num, den},
                                records_ask(&records_path, nullptr, kRmPlain, nullptr, 1, 0, precision, out_prefix, chatter, rate), records, n_records, nullptr, nullptr);
}

extern "C" int spsp_taxonomy_files_extract(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* lineages_path,
                                           uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix, int chatter, double rate,
                                           spsp_taxonomy_record** records, uint64_t* n_records, const char* what, int gz, uint64_t* n_kept,
                                           uint64_t* bytes_out) {
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }   // (in front of the clearing: DESIGN "What the record file drivers share")
    return taxonomy_files_entry({ctx, index_paths, lineages_path, true, false, n_ref, 0, min_keys, num, den},
                                records_ask(&records_path, nullptr, kRmExtract, what, gz, 0, precision, out_prefix, chatter, rate), records, n_records, n_kept, bytes_out);
}

extern "C" int spsp_taxonomy_files_paired(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path,
                                          const char* lineages_path, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix,
                                          int chatter, double rate, const char* what, int gz, spsp_taxonomy_record** records, uint64_t* n_records,
                                          uint64_t* n_kept, uint64_t* bytes_out) {
    return taxonomy_files_entry({ctx, index_paths, lineages_path, true, true, n_ref, 0, min_keys, num, den},
                                records_ask(&records_path, mates_path, what ? kRmExtract : kRmPlain, what, gz, 0, precision, out_prefix, chatter, rate), records, n_records,
                                n_kept, bytes_out);
}

extern "C" int spsp_taxonomy_files_split(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* records_path, const char* mates_path,
                                         const char* lineages_path, uint32_t min_keys, uint32_t num, uint32_t den, int precision, const char* out_prefix,
                                         int chatter, double rate, const char* what, int gz, spsp_taxonomy_record** records, uint64_t* n_records,
                                         uint64_t* n_bins_written, uint64_t* bytes_out) {
    if (!what) { set_error("NULL argument"); return SPSP_ERR_ARG; }   // (likewise)
    return taxonomy_files_entry({ctx, index_paths, lineages_path, true, false, n_ref, 0, min_keys, num, den},
                                records_ask(&records_path, mates_path, kRmSplit, what, gz, 0, precision, out_prefix, chatter, rate), records, n_records, n_bins_written,
                                bytes_out);
}

extern "C" int spsp_taxonomy_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    ctx->tx_clock.hand_out(ms);
    return SPSP_OK;
}
