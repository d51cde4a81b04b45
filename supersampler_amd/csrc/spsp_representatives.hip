// Representatives on the GPU: greedy dereplication of a collection from the cells of its pair matrix (not in the reference,
// whose end product is the two n x n matrices).  The other rule beside spsp_cluster.hip's single linkage: the one that
// promises that no two representatives are within the threshold of each other and that every member is within the threshold
// of the representative it is filed under.
//
// Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, w_i its weight (the caller's, or c_i), a cell
// i << 48 | j << 32 | x_ij names the keys two sketches share.  The link test is spsp_cluster.hip's, to the letter.  a comes
// before b iff w_a > w_b, or w_a == w_b and a < b: as one word, prio = w << 16 | 0xFFFF - i, larger first.  Going through the
// sketches in that order, a sketch is a REPRESENTATIVE iff it is linked to no representative before it (the lexicographically
// first maximal independent set of the link graph); every other sketch goes to the best of the representatives it is linked
// to, by the fraction x / u in 128-bit cross products, the earlier representative where two fractions are equal.
//
// The chain of launches:
//   k_rp_init     a lane per sketch: state = UNDECIDED, prio, best = 0, size = 0, first = none; the counter words
//   k_rp_edges    a lane per cell (tiles of 2048, grid-stride): range check, the link test, and for a link ONE 32-bit word
//                 first << 16 | second (the end that comes first in the high half) appended to the edge list: one atomicAdd
//                 per wave (ballot + popcount).  The list has room for n_cells words: no host wait sizes it
//   rounds        k_rp_round_edges (a lane per edge) + k_rp_round_nodes (a lane per sketch), queued in batches of 32, 64, ...,
//                 1024 rounds with ONE host wait per batch, for the count of undecided sketches.  A launch behind the fixed
//                 point returns at its first load
//   k_rp_assign   a second pass over the cells, the same test: a link between a REP and an OUT end is a candidate for the OUT
//                 end; the best one is kept in one 64-bit word per member (x << 16 | rep) by a CAS loop
//   k_rp_number   a lane per sketch: rep[i], size[rep] += 1, first[rep] = min(first[rep], i)
//   k_rp_first    a lane per sketch: "is its cluster's first-listed member"
//   scan          launch_scan_u32 over those flags: the cluster number in first-member order, and the cluster count
//   k_rp_rows     a lane per sketch: the 24-byte row
// and one host wait at the end, for the rows and the count.
//
// Why the rounds are right without a barrier.  Round r: over the edges (a, b), a first -- state[a] == REP: state[b] = OUT;
// state[a] == UNDECIDED and state[b] == UNDECIDED: blocked[b] = r.  Then, in a launch of its own, over the sketches --
// UNDECIDED and blocked != r: REP.  A state only ever rises (UNDECIDED < REP < OUT, by atomicMax).  A sketch becomes OUT only
// behind an earlier neighbour that IS a representative and REP only when every earlier neighbour was read as OUT; OUT and REP
// are never taken back, so whatever a lane reads as OUT or REP is final and true, whichever launch wrote it.  What a lane may
// read late is a state another workgroup set to OUT in the SAME launch: it then sees UNDECIDED, blocks a sketch that could have
// gone on, and that sketch is decided a round later -- a stale UNDECIDED only delays.  Everything a decision rests on (REP
// states, the blocked stamps) was written by an earlier LAUNCH.  The first undecided sketch of the order has no undecided
// sketch in front of it: every round decides at least that one, and the REP set the rounds end with is the sequential rule's.
// No workgroup waits for another one and nothing spins.
//
// How many rounds.  REP states are written by k_rp_round_nodes alone, so along a path 0 - 1 - 2 - ... that follows the order,
// sketch 2t can become REP in round t + 1 at the earliest (2t - 1 must be OUT, which takes 2t - 2 being REP in an earlier
// round): a path of L sketches takes ceil(L / 2) rounds or more, L where no lane ever profits from a fresh OUT.  The reported
// round is the one in which the count of undecided sketches reached 0.
#include <algorithm>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kRpThreads = 256;                       // 4 waves
constexpr uint32_t kRpTile = 2048;                         // cells (edges) per workgroup and turn: 8 rounds of 256
constexpr uint32_t kRpBlocksPerCu = 8;
constexpr int kRpWeightBits = 47;                          // a weight takes 48 bits of prio and leaves the top bit alone, as `best` does in clustering
constexpr uint32_t kRpBatchFirst = 32, kRpBatchMax = 1024; // rounds queued per host wait: 32, 64, ..., 1024, 1024, ...
enum RpState : uint32_t { kRpUndecided = 0, kRpRep = 1, kRpOut = 2 };
constexpr uint32_t kRpNone = 0xFFFFFFFFu;
// the counter words at the head of the work area.  kRpwLive = the sketches still undecided: it starts at n and only ever falls (a
// state leaves UNDECIDED through an atomicMax whose answer says who was first: every decision is counted once), so a value read
// late is too large and never says "done" too early; kRpwRounds = the round in which it reached 0
enum RpWord : uint32_t { kRpwEdges = 0 /* u64: words 0-1 */, kRpwBad = 2, kRpwRounds = 3, kRpwLive = 4, kRpwWords = 8 };

__device__ __forceinline__ uint32_t rp_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ unsigned long long rp_under(uint32_t metric, unsigned long long ci, unsigned long long cj, unsigned long long x) {
    return metric == SPSP_CLUSTER_JACCARD ? ci + cj - x : (ci < cj ? ci : cj);
}

struct RpRule {
    unsigned long long num, den, u_max;                    // u_max = (2^64 - 1) / num: k_cl_link's guard
    uint32_t n, metric;
};

// cell c -> is it a link?  Raises the bad-cell word for i >= j or j >= n, before the indices are used
__device__ __forceinline__ bool rp_link(const RpRule& R, const unsigned long long* __restrict__ card, unsigned long long c, uint32_t* __restrict__ words,
                                        uint32_t* i_out, uint32_t* j_out, unsigned long long* u_out) {
    const uint32_t i = (uint32_t)(c >> 48), j = (uint32_t)(c >> 32) & 0xffffu;
    const unsigned long long x = c & 0xffffffffull;
    if (i >= j || j >= R.n) { if (words) atomicOr(words + kRpwBad, 1u); return false; }
    if (!x) return false;
    const unsigned long long u = rp_under(R.metric, card[i], card[j], x);
    *i_out = i; *j_out = j; *u_out = u;
    return u <= R.u_max && x * R.den >= R.num * u;
}

__global__ __launch_bounds__(256) void k_rp_init(uint32_t n, const unsigned long long* __restrict__ weight, uint32_t* __restrict__ state,
                                                 uint32_t* __restrict__ blocked, unsigned long long* __restrict__ prio,
                                                 unsigned long long* __restrict__ best, uint32_t* __restrict__ size, uint32_t* __restrict__ first,
                                                 uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < kRpwWords) words[i] = i == kRpwLive ? n : 0u;
    if (i >= n) return;
    state[i] = kRpUndecided; blocked[i] = 0u; best[i] = 0ull; size[i] = 0u; first[i] = kRpNone;
    prio[i] = weight[i] << 16 | (unsigned long long)(0xFFFFu - i);
}

__global__ __launch_bounds__(kRpThreads) void k_rp_edges(const unsigned long long* __restrict__ cells, unsigned long long n_cells,
                                                         const unsigned long long* __restrict__ card, const unsigned long long* __restrict__ prio,
                                                         RpRule R, uint32_t* __restrict__ edges, uint32_t* __restrict__ words) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long n_tiles = (n_cells + kRpTile - 1) / kRpTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kRpTile / kRpThreads; ++r) {
            const unsigned long long e = tile * kRpTile + r * kRpThreads + threadIdx.x;
            bool edge = false;
            uint32_t i = 0, j = 0;
            unsigned long long u = 0;
            if (e < n_cells) edge = rp_link(R, card, cells[e], words, &i, &j, &u);
            const unsigned long long mask = __ballot(edge);   // (every lane of the wave is here)
            if (!mask) continue;
            unsigned long long base = 0;
            if (lane == (uint32_t)__ffsll((long long)mask) - 1u)
                base = atomicAdd(reinterpret_cast<unsigned long long*>(words + kRpwEdges), (unsigned long long)__popcll(mask));
            base = __shfl(base, __ffsll((long long)mask) - 1);
            // base + popcount(mask) <= the links among the cells <= n_cells: the list's room
            if (edge) edges[base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull))] = prio[i] > prio[j] ? i << 16 | j : j << 16 | i;
        }
    }
}

// the sketches this wave has just decided leave the count of the undecided: one atomic per wave, and the wave that takes the
// last ones away writes down the round it happened in
__device__ __forceinline__ void rp_decided(bool mine, uint32_t round, uint32_t* __restrict__ words) {
    const unsigned long long mask = __ballot(mine);
    if (!mine || (threadIdx.x & 63u) != (uint32_t)__ffsll((long long)mask) - 1u) return;
    const uint32_t k = (uint32_t)__popcll(mask);
    if (atomicSub(words + kRpwLive, k) == k) atomicExch(words + kRpwRounds, round);
}

__global__ __launch_bounds__(kRpThreads) void k_rp_round_edges(const uint32_t* __restrict__ edges, uint32_t round, uint32_t* __restrict__ state,
                                                               uint32_t* __restrict__ blocked, uint32_t* __restrict__ words) {
    if (rp_load(words + kRpwLive) == 0u) return;               // (nobody is undecided any more; a count read late is too large: the launch runs for nothing)
    const unsigned long long n_edges = *reinterpret_cast<const unsigned long long*>(words + kRpwEdges);
    const unsigned long long n_tiles = (n_edges + kRpTile - 1) / kRpTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kRpTile / kRpThreads; ++r) {
            const unsigned long long e = tile * kRpTile + r * kRpThreads + threadIdx.x;
            bool out = false;
            if (e < n_edges) {
                const uint32_t w = edges[e], a = w >> 16, b = w & 0xffffu;
                if (rp_load(state + b) == kRpUndecided) {
                    const uint32_t sa = rp_load(state + a);
                    if (sa == kRpRep) out = atomicMax(state + b, (uint32_t)kRpOut) == kRpUndecided;   // (the first lane to put b out counts it)
                    else if (sa == kRpUndecided) blocked[b] = round;
                }
            }
            rp_decided(out, round, words);
        }
    }
}

__global__ __launch_bounds__(256) void k_rp_round_nodes(uint32_t n, uint32_t round, uint32_t* __restrict__ state, const uint32_t* __restrict__ blocked,
                                                        uint32_t* __restrict__ words) {
    if (rp_load(words + kRpwLive) == 0u) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool rep = false;
    // (atomicMax: a sketch that is OUT stays OUT whatever this lane read)
    if (i < n && state[i] == kRpUndecided && blocked[i] != round) rep = atomicMax(state + i, (uint32_t)kRpRep) == kRpUndecided;
    rp_decided(rep, round, words);
}

__global__ __launch_bounds__(kRpThreads) void k_rp_assign(const unsigned long long* __restrict__ cells, unsigned long long n_cells,
                                                          const unsigned long long* __restrict__ card, const unsigned long long* __restrict__ prio,
                                                          RpRule R, const uint32_t* __restrict__ state, unsigned long long* __restrict__ best) {
    const unsigned long long n_tiles = (n_cells + kRpTile - 1) / kRpTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kRpTile / kRpThreads; ++r) {
            const unsigned long long e = tile * kRpTile + r * kRpThreads + threadIdx.x;
            if (e >= n_cells) continue;
            const unsigned long long c = cells[e];
            uint32_t i, j;
            unsigned long long u;
            if (!rp_link(R, card, c, nullptr, &i, &j, &u)) continue;   // (k_rp_edges has raised the flag)
            const uint32_t si = state[i], sj = state[j];
            uint32_t rep, member;
            if (si == kRpRep && sj == kRpOut) { rep = i; member = j; }
            else if (sj == kRpRep && si == kRpOut) { rep = j; member = i; }
            else continue;
            const unsigned long long x = c & 0xffffffffull, cand = x << 16 | rep, c_m = card[member], p_rep = prio[rep];
            unsigned long long* slot = best + member;
            unsigned long long held = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                if (held) {
                    const uint32_t q = (uint32_t)(held & 0xFFFFull);   // (a representative some lane wrote: below n)
                    const unsigned long long xq = held >> 16;
                    const int cmp = fraction_cmp(x, u, xq, rp_under(R.metric, c_m, card[q], xq));
                    if (cmp < 0 || (cmp == 0 && p_rep <= prio[q])) break;   // the holder stays
                }
                const unsigned long long was = atomicCAS(slot, held, cand);
                if (was == held) break;
                held = was;                                // somebody else got in: against the new holder, which is better than the old
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_rp_number(uint32_t n, const uint32_t* __restrict__ state, const unsigned long long* __restrict__ best,
                                                   uint32_t* __restrict__ rep_of, uint32_t* __restrict__ size, uint32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = best[i];
    // (every sketch that is not REP has a candidate, or a cell was bad and the call is refused: itself, then)
    const uint32_t rep = state[i] == kRpOut && b ? (uint32_t)(b & 0xFFFFull) : i;
    rep_of[i] = rep;
    atomicAdd(size + rep, 1u);
    atomicMin(first + rep, i);
}

__global__ __launch_bounds__(256) void k_rp_first(uint32_t n, const uint32_t* __restrict__ rep_of, const uint32_t* __restrict__ first,
                                                  uint32_t* __restrict__ is_first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) is_first[i] = first[rep_of[i]] == i ? 1u : 0u;
}

// number[i] for a first member i = the first members in front of it
__global__ __launch_bounds__(256) void k_rp_rows(uint32_t n, const unsigned long long* __restrict__ card, const uint32_t* __restrict__ rep_of,
                                                 const uint32_t* __restrict__ size, const uint32_t* __restrict__ first,
                                                 const uint32_t* __restrict__ number, const unsigned long long* __restrict__ best,
                                                 spsp_cluster_row* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t rep = rep_of[i];
    spsp_cluster_row row;
    row.cluster = number[first[rep]]; row.representative = rep; row.size = size[rep]; row.reserved = 0;
    row.shared = rep == i ? card[i] : best[i] >> 16;
    rows[i] = row;
}

}  // namespace

int representatives_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, const uint64_t* h_weight, uint32_t n,
                               int metric, uint32_t num, uint32_t den, spsp_cluster_row* rows, uint64_t* n_clusters, uint64_t* n_edges, uint32_t* n_rounds) {
    int rc;
    *n_clusters = 0; *n_edges = 0;
    if (n_rounds) *n_rounds = 0;
    if ((rc = cluster_check_args(n, metric, num, den))) return rc;
    if (n_cells && !d_cells) { set_error("NULL cell list"); return SPSP_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i) {
        if (h_card[i] >> kRpWeightBits) { set_error("sketch %u has %llu keys: representatives take key counts below 2^%d", i, (unsigned long long)h_card[i], kRpWeightBits); return SPSP_ERR_ARG; }
        if (h_weight && h_weight[i] >> kRpWeightBits) { set_error("sketch %u has weight %llu: representatives take weights below 2^%d", i, (unsigned long long)h_weight[i], kRpWeightBits); return SPSP_ERR_ARG; }
    }
    // work area: counter words | card, weight, prio, best (u64 x n) | state, blocked, size, first, rep_of (u32 x n) | is_first (u32 x (n + 1)) | number (u32 x (n + 2))
    const size_t n8 = (size_t)n * 8, n4 = ((size_t)n * 4 + 7) & ~(size_t)7;
    if ((rc = ctx->rp_work.reserve(64 + 4 * n8 + 7 * n4 + 64)) || (rc = ctx->rp_rows.reserve((size_t)n * sizeof(spsp_cluster_row))) ||
        (rc = ctx->rp_edges.reserve((size_t)std::max<uint64_t>(n_cells, 1) * 4))) return rc;
    uint8_t* w = ctx->rp_work.as<uint8_t>();
    uint32_t* d_words = reinterpret_cast<uint32_t*>(w);
    unsigned long long* d_card = reinterpret_cast<unsigned long long*>(w + 64);
    unsigned long long *d_weight = d_card + n, *d_prio = d_weight + n, *d_best = d_prio + n;
    uint8_t* w4 = w + 64 + 4 * n8;
    uint32_t* d_state = reinterpret_cast<uint32_t*>(w4);
    uint32_t* d_blocked = reinterpret_cast<uint32_t*>(w4 + n4);
    uint32_t* d_size = reinterpret_cast<uint32_t*>(w4 + 2 * n4);
    uint32_t* d_first = reinterpret_cast<uint32_t*>(w4 + 3 * n4);
    uint32_t* d_repof = reinterpret_cast<uint32_t*>(w4 + 4 * n4);
    uint32_t* d_isfirst = reinterpret_cast<uint32_t*>(w4 + 5 * n4);
    uint32_t* d_number = reinterpret_cast<uint32_t*>(w4 + 6 * n4 + 8);
    uint32_t* d_edges = ctx->rp_edges.as<uint32_t>();
    spsp_cluster_row* d_rows = ctx->rp_rows.as<spsp_cluster_row>();
    const unsigned long long* cells = reinterpret_cast<const unsigned long long*>(d_cells);
    RpRule R;
    R.num = num; R.den = den; R.u_max = ~0ull / num; R.n = n; R.metric = (uint32_t)metric;
    const uint32_t per_sketch = (n + 255) / 256;
    const uint64_t max_blocks = (uint64_t)std::max(ctx->n_cu, 1) * kRpBlocksPerCu;
    const uint32_t per_cell = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_cells + kRpTile - 1) / kRpTile, max_blocks));
    SPSP_HIP(hipMemcpyAsync(d_card, h_card, n8, hipMemcpyHostToDevice, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(d_weight, h_weight ? h_weight : h_card, n8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_rp_init, dim3(per_sketch), dim3(256), 0, ctx->stream, n, (const unsigned long long*)d_weight, d_state, d_blocked, d_prio, d_best, d_size,
                       d_first, d_words);
    hipLaunchKernelGGL(k_rp_edges, dim3(per_cell), dim3(kRpThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, (const unsigned long long*)d_card,
                       (const unsigned long long*)d_prio, R, d_edges, d_words);
    SPSP_HIP(hipGetLastError());
    // the rounds: the grid of the edge pass covers the cells until the first wait has told the edges
    uint32_t per_edge = per_cell, done = 0, batch = kRpBatchFirst;
    for (;;) {
        for (uint32_t s = 0; s < batch; ++s) {
            const uint32_t round = done + s + 1;
            hipLaunchKernelGGL(k_rp_round_edges, dim3(per_edge), dim3(kRpThreads), 0, ctx->stream, (const uint32_t*)d_edges, round, d_state, d_blocked,
                               d_words);
            hipLaunchKernelGGL(k_rp_round_nodes, dim3(per_sketch), dim3(256), 0, ctx->stream, n, round, d_state, (const uint32_t*)d_blocked, d_words);
        }
        SPSP_HIP(hipGetLastError());
        done += batch;
        SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsRpUndecided, d_words + kRpwLive, 4, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsRpEdges, d_words + kRpwEdges, 8, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsRpBad, d_words + kRpwBad, 8, hipMemcpyDeviceToHost, ctx->stream));   // the bad-cell word | the round that decided the last sketch << 32
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // one wait per batch of rounds (h_card and h_weight have been read by then)
        if ((uint32_t)ctx->h_scalar[kHsRpBad]) {
            set_error("a cell names a sketch outside the collection (or a pair that is not i < j)");
            memset(rows, 0, (size_t)n * sizeof(spsp_cluster_row));
            return SPSP_ERR_ARG;
        }
        if ((uint32_t)ctx->h_scalar[kHsRpUndecided] == 0) break;
        per_edge = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((ctx->h_scalar[kHsRpEdges] + kRpTile - 1) / kRpTile, max_blocks));
        batch = std::min(kRpBatchMax, batch * 2);
    }
    hipLaunchKernelGGL(k_rp_assign, dim3(per_cell), dim3(kRpThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, (const unsigned long long*)d_card,
                       (const unsigned long long*)d_prio, R, (const uint32_t*)d_state, d_best);
    hipLaunchKernelGGL(k_rp_number, dim3(per_sketch), dim3(256), 0, ctx->stream, n, (const uint32_t*)d_state, (const unsigned long long*)d_best, d_repof, d_size,
                       d_first);
    hipLaunchKernelGGL(k_rp_first, dim3(per_sketch), dim3(256), 0, ctx->stream, n, (const uint32_t*)d_repof, (const uint32_t*)d_first, d_isfirst);
    SPSP_HIP(hipGetLastError());
    if ((rc = launch_scan_u32(ctx, d_isfirst, d_number, n, ctx->h_scalar + kHsRpCount))) return rc;
    hipLaunchKernelGGL(k_rp_rows, dim3(per_sketch), dim3(256), 0, ctx->stream, n, (const unsigned long long*)d_card, (const uint32_t*)d_repof,
                       (const uint32_t*)d_size, (const uint32_t*)d_first, (const uint32_t*)d_number, (const unsigned long long*)d_best, d_rows);
    SPSP_HIP(hipGetLastError());
    SPSP_HIP(hipMemcpyAsync(rows, d_rows, (size_t)n * sizeof(spsp_cluster_row), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the last wait: the rows and the count
    *n_edges = ctx->h_scalar[kHsRpEdges];
    *n_clusters = (uint32_t)ctx->h_scalar[kHsRpCount];
    if (n_rounds) *n_rounds = (uint32_t)(ctx->h_scalar[kHsRpBad] >> 32);
    return SPSP_OK;
}

// spsp_representatives_files behind its argument checks: the sketches loaded (spsp_host.cpp), the all-vs-all as cells in
// ctx->m_cells, the pass over them, <out_prefix>_representatives.csv.gz
static int representatives_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den,
                                 const uint64_t* h_weight, const char* out_prefix, int chatter, double rate, std::vector<spsp_cluster_row>* rows,
                                 uint64_t* n_clusters) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "representatives are"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    std::vector<uint64_t>& card = run.card;
    uint64_t n_cells = 0, n_edges = 0;
    uint32_t n_rounds = 0;
    const DecodedKeys& keys = run.keys;
    rc = run.decode();
    if (!rc && keys.sk_off[n] && n > 1) rc = compare_keys_cells(ctx, keys, n, n, &n_cells);
    if (!rc) {
        rows->resize(n);
        rc = representatives_cells_impl(ctx, ctx->m_cells.as<uint64_t>(), n_cells, card.data(), h_weight, n, metric, num, den, rows->data(), n_clusters, &n_edges,
                                        &n_rounds);
    }
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_cluster_csv_host(rows->data(), paths, n, card.data(), metric, precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_representatives.csv.gz", t1)) || !chatter) return rc;
    uint32_t largest = 0;
    for (const spsp_cluster_row& r : *rows) largest = std::max(largest, r.size);
    printf("%u sketches, %llu edges, %llu representatives, the largest cluster of %u, %u rounds\n", n, (unsigned long long)n_edges,
           (unsigned long long)*n_clusters, largest, n_rounds);
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_representatives_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, const uint64_t* h_weight,
                                                 uint32_t n, int metric, uint32_t num, uint32_t den, spsp_cluster_row* rows, uint64_t* n_clusters,
                                                 uint64_t* n_edges, uint32_t* n_rounds) {
    if (!ctx || !h_card || !rows || !n_clusters || !n_edges) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return representatives_cells_impl(ctx, (const uint64_t*)d_cells, n_cells, h_card, h_weight, n, metric, num, den, rows, n_clusters, n_edges, n_rounds);
}

extern "C" int spsp_representatives_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den,
                                          const uint64_t* h_weight, const char* out_prefix, int chatter, double rate, spsp_cluster_row** rows,
                                          uint64_t* n_clusters) {
    if (rows) *rows = nullptr;
    if (n_clusters) *n_clusters = 0;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = cluster_check_args(n, metric, num, den))) return rc;
    if (h_weight)
        for (uint32_t i = 0; i < n; ++i)
            if (h_weight[i] >> kRpWeightBits) { set_error("sketch %u has weight %llu: representatives take weights below 2^%d", i, (unsigned long long)h_weight[i], kRpWeightBits); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_cluster_row> got;
    uint64_t count = 0;
    if ((rc = representatives_files(ctx, paths, n, precision, metric, num, den, h_weight, out_prefix, chatter, rate, &got, &count))) return rc;
    if (n_clusters) *n_clusters = count;
    return rows ? give_rows(got, rows) : SPSP_OK;
}
