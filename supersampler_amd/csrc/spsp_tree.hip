// The linkage tree on the GPU: the single-linkage dendrogram of a collection from the cells of its pair matrix (not in the
// reference, whose end product is the two n x n matrices).  The single-linkage hierarchy of a graph is its maximum spanning
// forest; the forest's edges, best first, are the merges, and cutting them at a threshold leaves the clusters spsp_cluster.hip
// reports at that threshold.  One pass over the cells answers every threshold at or above the floor.
//
// Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, a cell i << 48 | j << 32 | x names the keys two sketches
// share.  A cell is a CANDIDATE iff it passes spsp_cluster.hip's link test at the floor num / den (num == 0: every cell with
// x >= 1).  Edge a comes BEFORE edge b iff x_a / u_a > x_b / u_b in 128-bit cross products, or the fractions are equal and
// (i_a, j_a) < (i_b, j_b): a strict total order.  The forest is Kruskal's over the candidates in that order.
//
// Boruvka's algorithm in that order.  The chain of launches:
//   k_tr_init     a lane per sketch: parent[i] = i, root[i] = i, best[i] = 0; the counter words
//   k_tr_edges    a lane per cell (tiles of 2048, grid-stride): range check, the candidate test, and for a candidate the 8-byte
//                 cell word itself appended to list 0: the places by ballot + popcount per wave and ONE atomicAdd per
//                 workgroup and tile (24 bytes of LDS).  Each of the two lists has room for n_cells words: no host wait sizes them
//   rounds        floor(log2 n) of them, queued at once, three launches each:
//     k_tr_pick     a lane per edge of the round's list (its length is read from a device word): ri = root[i], rj = root[j]
//                   from the snapshot the last launch wrote.  ri == rj: the edge is inside a component and is dropped.  Else it
//                   is appended to the OTHER list (what the next round reads) and offered to best[ri] and best[rj]: one 64-bit
//                   word each, the cell word of the best edge so far, 0 = none -- a relaxed load, the order above against the
//                   holder, an atomicCAS only when the candidate comes before it, on from the word the CAS returns.
//                   The lanes of a wave that offer to one word settle it among themselves first (a butterfly of shuffles) and
//                   send one edge: the last rounds, where every edge lies between the same few components, stay cheap
//     k_tr_hook     a lane per sketch r that is a root with best[r] != 0: r' = the root of the edge's other end.  The edge is
//                   written to forest[atomicAdd(count)] iff best[r'] != best[r] || r < r' (a mutual choice is written once),
//                   and r and r' are united (spsp_device.h: cl_union, the larger root under the smaller)
//     k_tr_flatten  a lane per sketch: root[i] = find(i), best[i] = 0; one lane empties the list the round has read and counts
//                   the round if it hooked anything
// and ONE host wait at the end, for the forest's cell words, its count, the rounds and the bad-cell word.  The at most n - 1 forest
// edges are put into the order above, and given their sizes, on the host (spsp_host.cpp: tree_rows_host).
//
// Strict order means no cycle.  Let C be a component of a round and e the first edge, in the order, among the live edges that
// leave C.  Every other edge across the cut (C, rest) comes after e, so Kruskal meets e first; if e's ends were connected by
// then, the connecting path would cross the cut by an edge before e: there is none.  e is in the forest -- every edge a round
// chooses is, and the forest has no cycle, so the round's choices have none either.  Every component is connected by forest edges
// already (by induction over the rounds), so two DIFFERENT chosen edges between the same two components would close a cycle in
// the forest: the only edge two components can both choose is the same one.  best[r'] == best[r] is exactly "chosen twice", and
// r < r' writes it once.
//
// How many rounds.  A component with a live edge chooses one, and is united with the component at its other end, which has a live
// edge too (the same one at least).  So every component that has a live edge at the start of a round is, at its end, part of a
// component that holds two or more of them: the components with a live edge number at most n, then n / 2, n / 4, ...; one
// alone cannot have a live edge, so a round hooks something only while n / 2^t >= 2: floor(log2 n) rounds at most, 15 for
// n <= 65 535.  Exactly that many are queued; a round whose list is empty returns at its first load.
//
// What a decision rests on.  root[] and the lists' lengths were written by an earlier LAUNCH; nobody unites during k_tr_pick and
// nobody offers during k_tr_hook; best[] is zeroed by k_tr_flatten, not by the lanes that read their neighbour's word.  The
// exceptions are the CAS words (best[] in pick, parent[] in hook), which execute at the memory side.  No workgroup waits for
// another one and nothing spins on a value another lane is to write: a failed CAS means another lane's edge got in, the word
// only ever moves forward in a strict order, and the loser goes on from what the CAS returned.
#include <algorithm>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kTrThreads = 256;                       // 4 waves
constexpr uint32_t kTrTile = 2048;                         // cells (edges) per workgroup and turn: 8 rounds of 256
constexpr uint32_t kTrPer = kTrTile / kTrThreads;          // cells (edges) per lane and tile
constexpr uint32_t kTrBlocksPerCu = 8;
constexpr uint32_t kTrMaxDen = 1000000u;
constexpr int kTrCardBits = 47;                            // as clustering takes them: x * u stays below 2^80
// the counter words at the head of the work area.  kTrwLive: the lengths of the two edge lists (u64 each: words 0-1 and 2-3);
// kTrwEdges: the candidates, written down by the first round's pick before list 0 is emptied; kTrwBad | kTrwForest and
// kTrwRounds are copied to the host as they lie
enum TrWord : uint32_t { kTrwLive = 0, kTrwEdges = 4 /* u64 */, kTrwBad = 6, kTrwForest = 7, kTrwRounds = 8, kTrwWords = 16 };

__device__ __forceinline__ unsigned long long tr_under(uint32_t metric, unsigned long long ci, unsigned long long cj, unsigned long long x) {
    return metric == SPSP_CLUSTER_JACCARD ? ci + cj - x : (ci < cj ? ci : cj);
}

__device__ __forceinline__ unsigned long long* tr_len(uint32_t* words, uint32_t list) {
    return reinterpret_cast<unsigned long long*>(words + kTrwLive + 2u * list);
}

struct TrRule {
    unsigned long long num, den, u_max;                    // u_max = (2^64 - 1) / num: k_cl_link's guard (num == 0: no guard is needed)
    uint32_t n, metric;
};

__global__ __launch_bounds__(256) void k_tr_init(uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ root,
                                                 unsigned long long* __restrict__ best, uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < kTrwWords) words[i] = 0u;
    if (i >= n) return;
    parent[i] = i; root[i] = i; best[i] = 0ull;
}

// The appends of one workgroup and tile go through ONE atomicAdd on the list's length: a wave's own atomicAdd per 64 cells is
// 700 000 adds to one address over 4.5 x 10^7 cells, which queue at one memory channel and cost more than everything else in the
// pass.  flags: bit r = this lane's r-th cell of the tile is appended.  Counted per wave by ballot + popcount, summed over the
// four waves through 24 bytes of LDS, added once; every lane of the workgroup is here, and the barriers are the workgroup's own.
// -> the place of this WAVE's first append; tr_place then deals the places out, turn by turn.
struct TrShared { unsigned long long base; uint32_t wave[kTrThreads / 64]; };

__device__ __forceinline__ unsigned long long tr_reserve(uint32_t flags, unsigned long long* len, TrShared& sh) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < kTrPer; ++r) mine += (uint32_t)__popcll(__ballot((flags >> r) & 1u));
    __syncthreads();                                       // (the last tile's readers of sh are through)
    if (lane == 0) sh.wave[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < kTrThreads / 64; ++w) total += sh.wave[w];
        sh.base = total ? atomicAdd(len, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    unsigned long long base = sh.base;
    for (uint32_t w = 0; w < wave; ++w) base += sh.wave[w];
    return base;
}

// turn r of a tile: this lane's place if it appends (the wave's running place moves on by the wave's appends of the turn)
__device__ __forceinline__ unsigned long long tr_place(bool mine, unsigned long long* next) {
    const unsigned long long mask = __ballot(mine);        // (every lane of the wave is here)
    const unsigned long long at = *next + (unsigned long long)__popcll(mask & ((1ull << (threadIdx.x & 63u)) - 1ull));
    *next += (unsigned long long)__popcll(mask);
    return at;
}

__global__ __launch_bounds__(kTrThreads) void k_tr_edges(const unsigned long long* __restrict__ cells, unsigned long long n_cells,
                                                         const unsigned long long* __restrict__ card, TrRule R,
                                                         unsigned long long* __restrict__ list, uint32_t* __restrict__ words) {
    __shared__ TrShared sh;
    const unsigned long long n_tiles = (n_cells + kTrTile - 1) / kTrTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned long long c[kTrPer];
        uint32_t flags = 0;
#pragma unroll
        for (uint32_t r = 0; r < kTrPer; ++r) {
            const unsigned long long e = tile * kTrTile + r * kTrThreads + threadIdx.x;
            c[r] = 0;
            if (e < n_cells) {
                c[r] = cells[e];
                const uint32_t i = (uint32_t)(c[r] >> 48), j = (uint32_t)(c[r] >> 32) & 0xffffu;
                const unsigned long long x = c[r] & 0xffffffffull;
                if (i >= j || j >= R.n) atomicOr(words + kTrwBad, 1u);   // (tested before the indices are used; the call is refused)
                else if (x) {
                    const unsigned long long u = tr_under(R.metric, card[i], card[j], x);
                    if (u <= R.u_max && x * R.den >= R.num * u) flags |= 1u << r;
                }
            }
        }
        // the places: below the candidates among the cells <= n_cells: the list's room
        unsigned long long next = tr_reserve(flags, tr_len(words, 0), sh);
#pragma unroll
        for (uint32_t r = 0; r < kTrPer; ++r) {
            const bool edge = (flags >> r) & 1u;
            const unsigned long long at = tr_place(edge, &next);
            if (edge) list[at] = c[r];
        }
    }
}

// is edge a (x of u_a) before edge b in the order?  (a == b: no)
__device__ __forceinline__ bool tr_before(unsigned long long a, unsigned long long u_a, unsigned long long b, unsigned long long u_b) {
    const int cmp = fraction_cmp(a & 0xffffffffull, u_a, b & 0xffffffffull, u_b);
    return cmp > 0 || (cmp == 0 && (a >> 32) < (b >> 32));
}

// The lanes of a wave that offer to ONE word settle among themselves which edge comes first, and only that one goes to memory:
// in the last rounds every live edge lies between the same few components, and 64 loads and compare-and-swaps of one address per
// wave-instruction become one.  Every lane of the wave is here; `mine`: this lane takes part with edge c (u its denominator).
// -> is this lane's edge the first of those that take part?  (A butterfly over a strict total order: every lane ends with the
// same edge.)
__device__ __forceinline__ bool tr_wave_first(bool mine, unsigned long long c, unsigned long long u) {
    unsigned long long bc = mine ? c : 0ull, bu = u;       // 0: none
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long oc = __shfl_xor(bc, d), ou = __shfl_xor(bu, d);
        if (oc && (!bc || tr_before(oc, ou, bc, bu))) { bc = oc; bu = ou; }
    }
    return mine && bc == c;
}

// ... for up to four words per wave-instruction: the word of the first lane not yet dealt with, and every lane that offers to the
// same one.  A lane that loses to another lane's edge need not offer: that edge is offered to the same word in this launch.
// t: the root this lane offers to (live lanes only); -> does this lane still have to offer?  (Every lane of the wave is here.)
__device__ __forceinline__ bool tr_settle(bool live, uint32_t t, unsigned long long c, unsigned long long u) {
    const uint32_t lane = threadIdx.x & 63u;
    bool offer = live;
    unsigned long long rem = __ballot(live);
#pragma unroll 1
    for (int it = 0; it < 4 && rem; ++it) {
        const uint32_t lead = __shfl(t, __ffsll((long long)rem) - 1);
        const bool same = live && ((rem >> lane) & 1ull) && t == lead;
        const unsigned long long m = __ballot(same);       // (the first lane of rem is in it: rem shrinks)
        if (__popcll(m) >= 2 && !tr_wave_first(same, c, u) && same) offer = false;
        rem &= ~m;
    }
    return offer;
}

// edge c (x of u) is offered to one component's best-edge word: it gets in iff it comes before the holder in the order
__device__ __forceinline__ void tr_offer(unsigned long long* slot, unsigned long long c, unsigned long long x, unsigned long long u, uint32_t metric,
                                         const unsigned long long* __restrict__ card) {
    unsigned long long held = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        if (held) {
            // (an edge some lane wrote: its indices are below n)
            const unsigned long long xh = held & 0xffffffffull, uh = tr_under(metric, card[held >> 48], card[(held >> 32) & 0xffffull], xh);
            const int cmp = fraction_cmp(x, u, xh, uh);
            if (cmp < 0 || (cmp == 0 && (c >> 32) >= (held >> 32))) break;   // the holder stays (or is this very edge)
        }
        const unsigned long long was = atomicCAS(slot, held, c);
        if (was == held) break;
        held = was;                                        // somebody else got in: against the new holder, which comes before the old
    }
}

__global__ __launch_bounds__(kTrThreads) void k_tr_pick(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out, uint32_t src,
                                                        uint32_t first, const uint32_t* __restrict__ root, unsigned long long* __restrict__ best,
                                                        const unsigned long long* __restrict__ card, uint32_t metric, uint32_t* __restrict__ words) {
    const unsigned long long n_live = *tr_len(words, src);     // (written by an earlier launch)
    if (first && blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<unsigned long long*>(words + kTrwEdges) = n_live;
    if (!n_live) return;
    __shared__ TrShared sh;
    const unsigned long long n_tiles = (n_live + kTrTile - 1) / kTrTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned long long c[kTrPer];
        uint32_t flags = 0;
#pragma unroll
        for (uint32_t r = 0; r < kTrPer; ++r) {
            const unsigned long long e = tile * kTrTile + r * kTrThreads + threadIdx.x;
            c[r] = 0;
            if (e < n_live) {
                c[r] = in[e];
                // plain loads: nobody unites during this launch
                if (root[c[r] >> 48] != root[(c[r] >> 32) & 0xffffull]) flags |= 1u << r;
            }
        }
        // the places: below the live edges of this list <= its length <= n_cells: the other list's room
        unsigned long long next = tr_reserve(flags, tr_len(words, src ^ 1u), sh);
#pragma unroll 1
        for (uint32_t r = 0; r < kTrPer; ++r) {
            const bool live = (flags >> r) & 1u;
            if (!__ballot(live)) continue;                 // (the whole wave goes on, or none of it)
            const unsigned long long at = tr_place(live, &next), e = c[r];
            unsigned long long x = 0, u = 0;
            uint32_t ri = 0, rj = 0;
            if (live) {
                out[at] = e;
                ri = root[e >> 48]; rj = root[(e >> 32) & 0xffffull];
                x = e & 0xffffffffull;
                u = tr_under(metric, card[e >> 48], card[(e >> 32) & 0xffffull], x);
            }
            const bool to_i = tr_settle(live, ri, e, u), to_j = tr_settle(live, rj, e, u);
            if (to_i) tr_offer(best + ri, e, x, u, metric, card);
            if (to_j) tr_offer(best + rj, e, x, u, metric, card);
        }
    }
}

__global__ __launch_bounds__(256) void k_tr_hook(uint32_t n, uint32_t dst, const uint32_t* __restrict__ root, const unsigned long long* __restrict__ best,
                                                 uint32_t* __restrict__ parent, unsigned long long* __restrict__ forest, uint32_t* __restrict__ words) {
    if (*tr_len(words, dst) == 0ull) return;               // (no edge left between two components: nobody was offered one)
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n || root[r] != r) return;
    const unsigned long long c = best[r];
    if (!c) return;
    const uint32_t ri = root[c >> 48], rj = root[(c >> 32) & 0xffffull], other = ri == r ? rj : ri;
    if (best[other] != c || r < other) {
        const uint32_t at = atomicAdd(words + kTrwForest, 1u);
        if (at < n) forest[at] = c;                        // (a forest over n sketches has n - 1 edges at the most)
    }
    cl_union(parent, r, other);
}

__global__ __launch_bounds__(256) void k_tr_flatten(uint32_t n, uint32_t src, uint32_t* __restrict__ parent, uint32_t* __restrict__ root,
                                                    unsigned long long* __restrict__ best, uint32_t* __restrict__ words) {
    const bool hooked = *tr_len(words, src ^ 1u) != 0ull;  // an edge between two components: both of them chose one
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) {
        *tr_len(words, src) = 0ull;                        // the list this round has read is the one the next round fills
        if (hooked) words[kTrwRounds] += 1u;
    }
    if (!hooked || i >= n) return;
    root[i] = cl_find(parent, i, cl_load(parent + i));     // (no union runs any more: the roots stand still)
    best[i] = 0ull;
}

}  // namespace

int tree_check_args(uint32_t n, int metric, uint32_t num, uint32_t den) {
    int rc;
    if ((rc = cluster_check_args(n, metric, 1, 1))) return rc;
    if (den == 0 || num > den || den > kTrMaxDen) { set_error("tree floor %u / %u: needs 0 <= num <= den, 1 <= den <= %u", num, den, kTrMaxDen); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

// what the call refuses before it looks at its context: n, the metric, the floor, the key counts
static int tree_check_call(uint32_t n, int metric, uint32_t num, uint32_t den, const uint64_t* h_card) {
    int rc;
    if ((rc = tree_check_args(n, metric, num, den))) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (h_card[i] >> kTrCardBits) { set_error("sketch %u has %llu keys: the linkage tree takes key counts below 2^%d", i, (unsigned long long)h_card[i], kTrCardBits); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

int tree_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric, uint32_t num, uint32_t den,
                    spsp_tree_row* rows, uint64_t* n_rows, uint64_t* n_edges, uint32_t* n_rounds) {
    int rc;
    *n_rows = 0; *n_edges = 0;
    if (n_rounds) *n_rounds = 0;
    if ((rc = tree_check_call(n, metric, num, den, h_card))) return rc;
    if (n_cells && !d_cells) { set_error("NULL cell list"); return SPSP_ERR_ARG; }
    if (n > 1 && !rows) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    // work area: counter words | card, best (u64 x n) | parent, root (u32 x n)
    const size_t n8 = (size_t)n * 8, n4 = ((size_t)n * 4 + 7) & ~(size_t)7;
    const size_t room = (size_t)std::max<uint64_t>(n_cells, 1);
    if ((rc = ctx->tr_work.reserve(64 + 2 * n8 + 2 * n4)) || (rc = ctx->tr_forest.reserve(n8)) || (rc = ctx->tr_edges.reserve(2 * room * 8))) return rc;
    uint8_t* w = ctx->tr_work.as<uint8_t>();
    uint32_t* d_words = reinterpret_cast<uint32_t*>(w);
    unsigned long long* d_card = reinterpret_cast<unsigned long long*>(w + 64);
    unsigned long long* d_best = d_card + n;
    uint32_t* d_parent = reinterpret_cast<uint32_t*>(w + 64 + 2 * n8);
    uint32_t* d_root = reinterpret_cast<uint32_t*>(w + 64 + 2 * n8 + n4);
    unsigned long long* d_list[2] = {ctx->tr_edges.as<unsigned long long>(), ctx->tr_edges.as<unsigned long long>() + room};
    unsigned long long* d_forest = ctx->tr_forest.as<unsigned long long>();
    const unsigned long long* cells = reinterpret_cast<const unsigned long long*>(d_cells);
    TrRule R;
    R.num = num; R.den = den; R.u_max = num ? ~0ull / num : ~0ull; R.n = n; R.metric = (uint32_t)metric;
    const uint32_t per_sketch = (n + 255) / 256;
    const uint64_t max_blocks = (uint64_t)std::max(ctx->n_cu, 1) * kTrBlocksPerCu;
    const uint32_t per_cell = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_cells + kTrTile - 1) / kTrTile, max_blocks));
    uint32_t rounds = 0;                                   // floor(log2 n): the rounds that can hook anything (the top of the file)
    while ((2u << rounds) <= n) ++rounds;
    SPSP_HIP(hipMemcpyAsync(d_card, h_card, n8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_tr_init, dim3(per_sketch), dim3(256), 0, ctx->stream, n, d_parent, d_root, d_best, d_words);
    hipLaunchKernelGGL(k_tr_edges, dim3(per_cell), dim3(kTrThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, (const unsigned long long*)d_card, R,
                       d_list[0], d_words);
    for (uint32_t t = 0; t < rounds; ++t) {
        const uint32_t src = t & 1u;
        hipLaunchKernelGGL(k_tr_pick, dim3(per_cell), dim3(kTrThreads), 0, ctx->stream, (const unsigned long long*)d_list[src], d_list[src ^ 1u], src,
                           t == 0 ? 1u : 0u, (const uint32_t*)d_root, d_best, (const unsigned long long*)d_card, (uint32_t)metric, d_words);
        hipLaunchKernelGGL(k_tr_hook, dim3(per_sketch), dim3(256), 0, ctx->stream, n, src ^ 1u, (const uint32_t*)d_root, (const unsigned long long*)d_best,
                           d_parent, d_forest, d_words);
        hipLaunchKernelGGL(k_tr_flatten, dim3(per_sketch), dim3(256), 0, ctx->stream, n, src, d_parent, d_root, d_best, d_words);
    }
    SPSP_HIP(hipGetLastError());
    std::vector<uint64_t> forest(n);
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsTrEdges, d_words + kTrwEdges, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsTrBad, d_words + kTrwBad, 8, hipMemcpyDeviceToHost, ctx->stream));   // the bad-cell word | the forest's edges << 32
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsTrRounds, d_words + kTrwRounds, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 1) SPSP_HIP(hipMemcpyAsync(forest.data(), d_forest, (size_t)(n - 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait (h_card has been read by then)
    const uint64_t n_forest = ctx->h_scalar[kHsTrBad] >> 32;
    if ((uint32_t)ctx->h_scalar[kHsTrBad]) {
        set_error("a cell names a sketch outside the collection (or a pair that is not i < j)");
        if (n > 1) memset(rows, 0, (size_t)(n - 1) * sizeof(spsp_tree_row));
        return SPSP_ERR_ARG;
    }
    if (n_forest >= n) {                                   // (cannot be: the round's choices are forest edges)
        set_error("the linkage tree kept %llu edges over %u sketches", (unsigned long long)n_forest, n);
        if (n > 1) memset(rows, 0, (size_t)(n - 1) * sizeof(spsp_tree_row));
        return SPSP_ERR_OVERFLOW;
    }
    if ((rc = tree_rows_host(forest.data(), n_forest, h_card, n, metric, rows))) return rc;
    *n_rows = n_forest;
    *n_edges = ctx->h_scalar[kHsTrEdges];
    if (n_rounds) *n_rounds = (uint32_t)ctx->h_scalar[kHsTrRounds];
    return SPSP_OK;
}

// spsp_tree_files behind its argument checks: the sketches loaded (spsp_host.cpp), the all-vs-all as cells in ctx->m_cells, the
// pass over them, <out_prefix>_tree.csv.gz and <out_prefix>_tree.nwk
static int tree_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den, const char* out_prefix,
                      int chatter, double rate, std::vector<spsp_tree_row>* rows, uint64_t* n_rows) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "the linkage tree is"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    std::vector<uint64_t>& card = run.card;
    uint64_t n_cells = 0, n_edges = 0;
    uint32_t n_rounds = 0;
    const DecodedKeys& keys = run.keys;
    rc = run.decode();
    if (!rc && keys.sk_off[n] && n > 1) rc = compare_keys_cells(ctx, keys, n, n, &n_cells);
    if (!rc) {
        rows->resize(n - 1);
        rc = tree_cells_impl(ctx, ctx->m_cells.as<uint64_t>(), n_cells, card.data(), n, metric, num, den, rows->data(), n_rows, &n_edges, &n_rounds);
        if (!rc) rows->resize(*n_rows);
    }
    const double t1 = run.end();
    if (rc) return rc;
    char *csv = nullptr, *nwk = nullptr; uint64_t csv_len = 0, nwk_len = 0;
    if ((rc = spsp_tree_csv_host(rows->data(), *n_rows, paths, n, card.data(), metric, precision, &csv, &csv_len))) return rc;
    if ((rc = spsp_tree_newick_host(rows->data(), *n_rows, paths, n, card.data(), metric, precision, &nwk, &nwk_len))) { spsp_free(csv); return rc; }
    const std::string nwk_path = std::string(out_prefix) + "_tree.nwk";
    FILE* f = fopen(nwk_path.c_str(), "wb");
    const bool written = f && fwrite(nwk, 1, nwk_len, f) == nwk_len;
    const bool closed = f && fclose(f) == 0;
    spsp_free(nwk);
    if (!written || !closed) { spsp_free(csv); set_error("cannot write %s", nwk_path.c_str()); return SPSP_ERR_IO; }
    if ((rc = write_csv_gz(ctx, csv, csv_len, out_prefix, "_tree.csv.gz", t1)) || !chatter) return rc;
    printf("%u sketches, %llu candidate edges, %llu forest rows, %llu components left, %u rounds\n", n, (unsigned long long)n_edges,
           (unsigned long long)*n_rows, (unsigned long long)(n - *n_rows), n_rounds);
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_tree_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric, uint32_t num,
                                      uint32_t den, spsp_tree_row* rows, uint64_t* n_rows, uint64_t* n_edges, uint32_t* n_rounds) {
    if (n_rows) *n_rows = 0;
    if (n_edges) *n_edges = 0;
    if (n_rounds) *n_rounds = 0;
    if (!h_card || !n_rows || !n_edges) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = tree_check_call(n, metric, num, den, h_card))) return rc;   // (in front of the context: decided before any device is touched)
    if (!ctx) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return tree_cells_impl(ctx, (const uint64_t*)d_cells, n_cells, h_card, n, metric, num, den, rows, n_rows, n_edges, n_rounds);
}

extern "C" int spsp_tree_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den,
                               const char* out_prefix, int chatter, double rate, spsp_tree_row** rows, uint64_t* n_rows) {
    if (rows) *rows = nullptr;
    if (n_rows) *n_rows = 0;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = tree_check_args(n, metric, num, den))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_tree_row> got;
    uint64_t count = 0;
    if ((rc = tree_files(ctx, paths, n, precision, metric, num, den, out_prefix, chatter, rate, &got, &count))) return rc;
    if (n_rows) *n_rows = count;
    return rows ? give_rows(got, rows) : SPSP_OK;
}
