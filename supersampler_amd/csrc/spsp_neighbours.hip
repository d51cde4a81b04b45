// Neighbours on the GPU: each sketch's best few partners at or above a threshold, best first, from the cells of the pair
// matrix (not in the reference, whose end product is the two n x n matrices).
//
// Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, a cell i << 48 | j << 32 | x names the keys two
// sketches share.  Rows: every sketch (n_query == n; a cell serves both of its ends), or the queries 0 .. n_query-1 against
// the references n_query .. n-1 (a cell between two queries, or between two references, is nobody's).  The score of partner p
// for row r is the fraction x / u: u = c_r + c_p - x (Jaccard), min(c_r, c_p) (the larger containment) or c_r (the row's
// containment in the partner).  An end passes iff x >= 1 and x * den >= num * u; p comes before q iff x_p * u_q > x_q * u_p,
// the smaller index first where the two 128-bit products are equal.  Integers only: no float decides anything.
//
// One fixed chain of launches whatever n, n_cells and top are:
//   k_nb_init    a lane per row: deg = cursor = 0; the counter words
//   k_nb_count   a lane per cell (tiles of 2048, grid-stride): range check, the row filter, the pass test; deg[row] += 1 for
//                every end that passed; the cells with a passing end are counted per wave (ballot + popcount)
//   k_nb_cap     a lane per row: min(deg, top)
//   scan x 2     launch_scan_u32 over deg -> where each row's candidates go, and over min(deg, top) -> where its rows go
//   -- the first host wait: the two totals (they size the candidate list and the rows), the pair count, the bad-cell word --
//   k_nb_fill    the second pass over the cells, the same test: a passing end writes x << 16 | partner into its row's slice
//                through an atomic cursor.  The order inside a slice is whatever the lanes made it: nothing reads it as one
//   k_nb_select  a wave per row, four rows per workgroup: the row's best 64 candidates, one per lane, sorted; the slice is
//                streamed 64 at a time, each chunk sorted by a bitonic network of __shfl_xor compare-exchanges and merged with
//                the kept 64 (a bitonic merge of the 128 whose worse half is dropped); the first min(deg, top) lanes write the
//                rows at their final place.  No LDS
//   -- the second host wait: the rows --
// No workgroup waits for another one and nothing spins.  The cells are only read.
//
// Why the answer does not depend on arrival order: the order above is a strict total order on a row's passing partners (two
// different partners never compare equal: the index breaks every tie), so "the first top of them" is a property of the SET of
// candidates in the slice.  A chunk that holds nothing better than the 64th kept candidate is dropped unsorted: by the same
// argument it cannot change the best 64.
#include <algorithm>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kNbThreads = 256;                       // 4 waves
constexpr uint32_t kNbTile = 2048;                         // cells per workgroup and turn: 8 rounds of 256
constexpr uint32_t kNbBlocksPerCu = 8;
constexpr uint32_t kNbMaxDen = 1000000u;
constexpr uint32_t kNbMaxTop = 64;                         // the kept candidates of a row are one wave wide
constexpr int kNbCardBits = 47;                            // key counts below 2^47, as clustering takes them
// the counter words at the head of the work area
enum NbWord : uint32_t { kNbwPairs = 0 /* u64: words 0-1 */, kNbwBad = 2 /* u32 */, kNbwWords = 4 };

struct NbRule {
    unsigned long long num, den, u_max;                    // u_max = (2^64 - 1) / num (all ones for num == 0): see nb_pass
    uint32_t n, n_query, metric;
};

__device__ __forceinline__ unsigned long long nb_under(uint32_t metric, unsigned long long c_row, unsigned long long c_partner, unsigned long long x) {
    return metric == SPSP_NEIGHBOUR_JACCARD ? c_row + c_partner - x : metric == SPSP_NEIGHBOUR_CONTAINMENT ? (c_row < c_partner ? c_row : c_partner) : c_row;
}

// A right-hand side beyond 64 bits is larger than any left-hand side (x < 2^32, den <= 10^6: x * den < 2^52), so such an end does
// not pass and the product is never formed.
__device__ __forceinline__ bool nb_pass(const NbRule& R, unsigned long long x, unsigned long long u) { return u <= R.u_max && x * R.den >= R.num * u; }

// What one cell means to the two passes: which of its ends are rows and passed.  i < j < n has been checked.
__device__ __forceinline__ void nb_ends(const NbRule& R, const unsigned long long* __restrict__ card, uint32_t i, uint32_t j, unsigned long long x,
                                        bool* pass_i, bool* pass_j) {
    *pass_i = *pass_j = false;
    if (!x) return;
    const bool all = R.n_query == R.n;
    if (!all && (i >= R.n_query || j < R.n_query)) return;  // (query mode: a query and a reference, the query in front)
    const unsigned long long ci = card[i], cj = card[j];
    *pass_i = nb_pass(R, x, nb_under(R.metric, ci, cj, x));
    if (all) *pass_j = R.metric == SPSP_NEIGHBOUR_CONTAINED ? nb_pass(R, x, cj) : *pass_i;
}

__global__ __launch_bounds__(256) void k_nb_init(uint32_t n_rows, uint32_t* __restrict__ deg, uint32_t* __restrict__ cursor, uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < kNbwWords) words[i] = 0u;
    if (i >= n_rows) return;
    deg[i] = 0u; cursor[i] = 0u;
}

__global__ __launch_bounds__(kNbThreads) void k_nb_count(const unsigned long long* __restrict__ cells, unsigned long long n_cells,
                                                         const unsigned long long* __restrict__ card, NbRule R, uint32_t* __restrict__ deg,
                                                         uint32_t* __restrict__ words) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long n_tiles = (n_cells + kNbTile - 1) / kNbTile;
    unsigned long long pairs = 0;                          // of this wave (the same number in every lane)
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kNbTile / kNbThreads; ++r) {
            const unsigned long long e = tile * kNbTile + r * kNbThreads + threadIdx.x;
            bool pi = false, pj = false;
            uint32_t i = 0, j = 0;
            if (e < n_cells) {
                const unsigned long long c = cells[e];
                i = (uint32_t)(c >> 48); j = (uint32_t)(c >> 32) & 0xffffu;
                if (i >= j || j >= R.n) atomicOr(words + kNbwBad, 1u);   // (tested before the indices are used; the call is refused)
                else nb_ends(R, card, i, j, c & 0xffffffffull, &pi, &pj);
            }
            pairs += (unsigned long long)__popcll(__ballot(pi || pj));   // (every lane of the wave is here)
            if (pi) atomicAdd(deg + i, 1u);
            if (pj) atomicAdd(deg + j, 1u);
        }
    }
    if (lane == 0 && pairs) atomicAdd(reinterpret_cast<unsigned long long*>(words + kNbwPairs), pairs);
}

__global__ __launch_bounds__(256) void k_nb_cap(uint32_t n_rows, uint32_t top, const uint32_t* __restrict__ deg, uint32_t* __restrict__ capped) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_rows) capped[i] = deg[i] < top ? deg[i] : top;
}

// cand_off[row] + cursor stays below cand_off[row + 1]: k_nb_count counted the same ends by the same test over the same cells
__global__ __launch_bounds__(kNbThreads) void k_nb_fill(const unsigned long long* __restrict__ cells, unsigned long long n_cells,
                                                        const unsigned long long* __restrict__ card, NbRule R, const uint32_t* __restrict__ deg,
                                                        const uint32_t* __restrict__ cand_off, uint32_t* __restrict__ cursor,
                                                        unsigned long long* __restrict__ cand) {
    const unsigned long long n_tiles = (n_cells + kNbTile - 1) / kNbTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kNbTile / kNbThreads; ++r) {
            const unsigned long long e = tile * kNbTile + r * kNbThreads + threadIdx.x;
            if (e >= n_cells) continue;
            const unsigned long long c = cells[e];
            const uint32_t i = (uint32_t)(c >> 48), j = (uint32_t)(c >> 32) & 0xffffu;
            if (i >= j || j >= R.n) continue;              // (k_nb_count has raised the flag)
            const unsigned long long x = c & 0xffffffffull;
            bool pi, pj;
            nb_ends(R, card, i, j, x, &pi, &pj);
            if (pi) { const uint32_t at = atomicAdd(cursor + i, 1u); if (at < deg[i]) cand[(unsigned long long)cand_off[i] + at] = x << 16 | j; }
            if (pj) { const uint32_t at = atomicAdd(cursor + j, 1u); if (at < deg[j]) cand[(unsigned long long)cand_off[j] + at] = x << 16 | i; }
        }
    }
}

// One candidate of a row: w = x << 16 | partner, u = what x is divided by.  An empty lane holds w = 0xFFFF (x = 0, a partner no
// sketch has), u = 1: it loses to every candidate (x * 1 > 0 * u) and equals its like.
struct NbCand { unsigned long long w, u; };
constexpr unsigned long long kNbEmpty = 0xFFFFull;

// a strictly in front of b: x_a * u_b > x_b * u_a in 128 bits, the smaller partner where the products are equal
__device__ __forceinline__ bool nb_before(const NbCand& a, const NbCand& b) {
    const int cmp = fraction_cmp(a.w >> 16, a.u, b.w >> 16, b.u);
    return cmp ? cmp > 0 : (a.w & 0xFFFFull) < (b.w & 0xFFFFull);
}

__device__ __forceinline__ NbCand nb_from(const NbCand& v, uint32_t src_lane) {
    NbCand o;
    o.w = __shfl(v.w, (int)src_lane);
    o.u = __shfl(v.u, (int)src_lane);
    return o;
}

// one compare-exchange with the lane `j` away: the lane keeps the one in front (front == true) or the one behind
__device__ __forceinline__ void nb_exchange(NbCand& v, uint32_t j, bool front) {
    NbCand o;
    o.w = __shfl_xor(v.w, (int)j);
    o.u = __shfl_xor(v.u, (int)j);
    const bool take = front ? nb_before(o, v) : nb_before(v, o);
    if (take) v = o;
}

__global__ __launch_bounds__(256) void k_nb_select(uint32_t n, uint32_t n_rows, uint32_t metric, uint32_t top, const unsigned long long* __restrict__ card,
                                                   const uint32_t* __restrict__ deg, const uint32_t* __restrict__ cand_off,
                                                   const uint32_t* __restrict__ row_off, const unsigned long long* __restrict__ cand,
                                                   spsp_neighbour_row* __restrict__ rows) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);   // (the same in every lane of a wave: the shuffles below see whole waves)
    if (row >= n_rows) return;
    const uint32_t d = deg[row];
    if (!d) return;
    const unsigned long long c_row = card[row];
    const unsigned long long* mine = cand + cand_off[row];
    NbCand kept;
    kept.w = kNbEmpty; kept.u = 1ull;
    for (uint32_t base = 0; base < d; base += 64u) {
        NbCand v;
        v.w = kNbEmpty; v.u = 1ull;
        if (base + lane < d) {
            v.w = mine[base + lane];
            const uint32_t p = (uint32_t)(v.w & 0xFFFFull);                  // (k_nb_fill wrote an index below n; card is not read beyond its end whatever is there)
            v.u = nb_under(metric, c_row, p < n ? card[p] : 0ull, v.w >> 16);
        }
        // nothing here in front of the last one kept: the best 64 stay what they are
        if (!__any(nb_before(v, nb_from(kept, 63u)))) continue;
        // the chunk, best first: lane l keeps the front one of a pair when it is the pair's lower lane in a run that goes forward
#pragma unroll
        for (uint32_t k = 2; k <= 64u; k <<= 1)
#pragma unroll
            for (uint32_t j = k >> 1; j; j >>= 1) nb_exchange(v, j, ((lane & j) == 0) == ((lane & k) == 0));
        // kept (best first) against the chunk reversed: the front one of every pair -- the best 64 of the 128, as a bitonic run
        const NbCand o = nb_from(v, 63u - lane);
        if (nb_before(o, kept)) kept = o;
#pragma unroll
        for (uint32_t j = 32; j; j >>= 1) nb_exchange(kept, j, (lane & j) == 0);
    }
    const uint32_t out = d < top ? d : top;
    if (lane < out) {
        spsp_neighbour_row r;
        r.sketch = row; r.rank = lane + 1u; r.neighbour = (uint32_t)(kept.w & 0xFFFFull); r.reserved = 0u;
        r.shared = kept.w >> 16;
        rows[(unsigned long long)row_off[row] + lane] = r;
    }
}

}  // namespace

int neighbours_check_args(uint32_t n, uint32_t n_query, int metric, uint32_t num, uint32_t den, uint32_t top) {
    if (n == 0 || n > 65535) { set_error("neighbours take 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_query == 0 || n_query > n) { set_error("neighbours: %u queries of %u sketches (1 .. n; n = all versus all)", n_query, n); return SPSP_ERR_ARG; }
    if (metric != SPSP_NEIGHBOUR_JACCARD && metric != SPSP_NEIGHBOUR_CONTAINMENT && metric != SPSP_NEIGHBOUR_CONTAINED) {
        set_error("neighbour metric %d: 0 (Jaccard), 1 (the larger containment) or 2 (the row's containment in the partner)", metric);
        return SPSP_ERR_ARG;
    }
    if (num > den || den > kNbMaxDen) { set_error("neighbour threshold %u / %u: needs 0 <= num <= den <= %u", num, den, kNbMaxDen); return SPSP_ERR_ARG; }
    if (top == 0 || top > kNbMaxTop) { set_error("neighbours: the best %u per sketch (1 .. %u)", top, kNbMaxTop); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

int neighbours_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, uint32_t n_query, int metric,
                          uint32_t num, uint32_t den, uint32_t top, spsp_neighbour_row* rows, uint64_t cap, uint64_t* n_rows, uint32_t* passing,
                          uint64_t* n_pairs) {
    int rc;
    *n_rows = 0; *n_pairs = 0;
    if ((rc = neighbours_check_args(n, n_query, metric, num, den, top))) return rc;
    if (n_cells && !d_cells) { set_error("NULL cell list"); return SPSP_ERR_ARG; }
    if (cap && !rows) { set_error("NULL rows"); return SPSP_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i)
        if (h_card[i] >> kNbCardBits) { set_error("sketch %u has %llu keys: neighbours take key counts below 2^%d", i, (unsigned long long)h_card[i], kNbCardBits); return SPSP_ERR_ARG; }
    // the candidates of all rows are placed by a 32-bit scan: a cell list that could give 2^32 of them or more is refused here
    const bool all = n_query == n;
    if (n_cells >= (all ? 1ull << 31 : 1ull << 32)) {
        set_error("neighbours: %llu cells could give 2^32 candidates or more", (unsigned long long)n_cells);
        return SPSP_ERR_ARG;
    }
    const uint32_t nr = n_query;                           // rows: every sketch, or the queries
    // work area: counter words | card (u64 x n) | deg, cursor, capped (u32 x nr) | cand_off, row_off (u32 x (nr + 2))
    const size_t n8 = (size_t)n * 8, r4 = ((size_t)nr * 4 + 7) & ~(size_t)7, o4 = r4 + 8;
    if ((rc = ctx->nb_work.reserve(64 + n8 + 3 * r4 + 2 * o4 + 64))) return rc;
    uint8_t* w = ctx->nb_work.as<uint8_t>();
    uint32_t* d_words = reinterpret_cast<uint32_t*>(w);
    unsigned long long* d_card = reinterpret_cast<unsigned long long*>(w + 64);
    uint32_t* d_deg = reinterpret_cast<uint32_t*>(w + 64 + n8);
    uint32_t* d_cursor = reinterpret_cast<uint32_t*>(w + 64 + n8 + r4);
    uint32_t* d_capped = reinterpret_cast<uint32_t*>(w + 64 + n8 + 2 * r4);
    uint32_t* d_cand_off = reinterpret_cast<uint32_t*>(w + 64 + n8 + 3 * r4);
    uint32_t* d_row_off = reinterpret_cast<uint32_t*>(w + 64 + n8 + 3 * r4 + o4);
    const unsigned long long* cells = reinterpret_cast<const unsigned long long*>(d_cells);
    NbRule R;
    R.num = num; R.den = den; R.u_max = num ? ~0ull / num : ~0ull;
    R.n = n; R.n_query = n_query; R.metric = (uint32_t)metric;
    const uint32_t per_row = (nr + 255) / 256;
    const uint64_t tiles = (n_cells + kNbTile - 1) / kNbTile;
    const uint32_t per_cell = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)std::max(ctx->n_cu, 1) * kNbBlocksPerCu));
    SPSP_HIP(hipMemcpyAsync(d_card, h_card, n8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_nb_init, dim3(per_row), dim3(256), 0, ctx->stream, nr, d_deg, d_cursor, d_words);
    hipLaunchKernelGGL(k_nb_count, dim3(per_cell), dim3(kNbThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, (const unsigned long long*)d_card, R,
                       d_deg, d_words);
    hipLaunchKernelGGL(k_nb_cap, dim3(per_row), dim3(256), 0, ctx->stream, nr, top, (const uint32_t*)d_deg, d_capped);
    SPSP_HIP(hipGetLastError());
    if ((rc = launch_scan_u32(ctx, d_deg, d_cand_off, nr, ctx->h_scalar + kHsNbCands)) ||
        (rc = launch_scan_u32(ctx, d_capped, d_row_off, nr, ctx->h_scalar + kHsNbRows))) return rc;
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsNbPairs, d_words + kNbwPairs, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsNbBad, d_words + kNbwBad, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (passing) SPSP_HIP(hipMemcpyAsync(passing, d_deg, (size_t)nr * 4, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the first wait: the totals that size what follows (h_card has been read by then)
    if ((uint32_t)ctx->h_scalar[kHsNbBad]) {
        set_error("a cell names a sketch outside the collection (or a pair that is not i < j)");
        if (cap) memset(rows, 0, (size_t)cap * sizeof(spsp_neighbour_row));
        if (passing) memset(passing, 0, (size_t)nr * 4);
        return SPSP_ERR_ARG;
    }
    const uint64_t n_cand = (uint32_t)ctx->h_scalar[kHsNbCands], need = (uint32_t)ctx->h_scalar[kHsNbRows];
    *n_pairs = ctx->h_scalar[kHsNbPairs];
    *n_rows = need;
    if (need > cap) { set_error("neighbours: %llu rows, room for %llu", (unsigned long long)need, (unsigned long long)cap); return SPSP_ERR_OVERFLOW; }
    if (!need) return SPSP_OK;
    if ((rc = ctx->nb_cand.reserve((size_t)n_cand * 8)) || (rc = ctx->nb_rows.reserve((size_t)need * sizeof(spsp_neighbour_row)))) return rc;
    unsigned long long* d_cand = ctx->nb_cand.as<unsigned long long>();
    spsp_neighbour_row* d_rows = ctx->nb_rows.as<spsp_neighbour_row>();
    hipLaunchKernelGGL(k_nb_fill, dim3(per_cell), dim3(kNbThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, (const unsigned long long*)d_card, R,
                       (const uint32_t*)d_deg, (const uint32_t*)d_cand_off, d_cursor, d_cand);
    hipLaunchKernelGGL(k_nb_select, dim3((nr + 3) / 4), dim3(256), 0, ctx->stream, n, nr, (uint32_t)metric, top, (const unsigned long long*)d_card,
                       (const uint32_t*)d_deg, (const uint32_t*)d_cand_off, (const uint32_t*)d_row_off, (const unsigned long long*)d_cand, d_rows);
    SPSP_HIP(hipGetLastError());
    SPSP_HIP(hipMemcpyAsync(rows, d_rows, (size_t)need * sizeof(spsp_neighbour_row), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the second wait: the rows
    return SPSP_OK;
}

// spsp_neighbours_files behind its argument checks: the sketches loaded (spsp_host.cpp), the cells of the queries' rows (or of all
// rows) in ctx->m_cells, the neighbours pass over them, <out_prefix>_neighbours.csv.gz
static int neighbours_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, int metric, uint32_t num, uint32_t den,
                            uint32_t top, const char* out_prefix, int chatter, double rate, std::vector<spsp_neighbour_row>* rows) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "neighbours are"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    std::vector<uint64_t>& card = run.card;
    std::vector<uint32_t> passing(n_query, 0);
    uint64_t n_cells = 0, n_rows = 0, n_pairs = 0;
    const DecodedKeys& keys = run.keys;
    rc = run.decode();
    if (!rc && keys.sk_off[n] && n > 1) rc = compare_keys_cells(ctx, keys, n, n_query, &n_cells);
    if (!rc) {
        // room for every row there can be: at most `top` per row sketch, and no more than the cells have ends
        rows->resize((size_t)std::min<uint64_t>((uint64_t)n_query * top, 2 * n_cells));
        rc = neighbours_cells_impl(ctx, ctx->m_cells.as<uint64_t>(), n_cells, card.data(), n, n_query, metric, num, den, top, rows->data(), rows->size(), &n_rows,
                                   passing.data(), &n_pairs);
        rows->resize(rc ? 0 : (size_t)n_rows);
    }
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_neighbours_csv_host(rows->data(), n_rows, passing.data(), paths, n, n_query, card.data(), metric, precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_neighbours.csv.gz", t1)) || !chatter) return rc;
    printf("%u sketches, %llu passing pairs, %llu rows written\n", n, (unsigned long long)n_pairs, (unsigned long long)n_rows);
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_neighbours_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, uint32_t n_query,
                                            int metric, uint32_t num, uint32_t den, uint32_t top, spsp_neighbour_row* rows, uint64_t cap, uint64_t* n_rows,
                                            uint32_t* passing, uint64_t* n_pairs) {
    if (!ctx || !h_card || !n_rows || !n_pairs) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return neighbours_cells_impl(ctx, (const uint64_t*)d_cells, n_cells, h_card, n, n_query, metric, num, den, top, rows, cap, n_rows, passing, n_pairs);
}

extern "C" int spsp_neighbours_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, int metric, uint32_t num,
                                     uint32_t den, uint32_t top, const char* out_prefix, int chatter, double rate, spsp_neighbour_row** rows,
                                     uint64_t* n_rows) {
    if (rows) *rows = nullptr;
    if (n_rows) *n_rows = 0;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = neighbours_check_args(n, n_query, metric, num, den, top))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_neighbour_row> got;
    if ((rc = neighbours_files(ctx, paths, n, n_query, precision, metric, num, den, top, out_prefix, chatter, rate, &got))) return rc;
    if (n_rows) *n_rows = got.size();
    return rows ? give_rows(got, rows) : SPSP_OK;
}
