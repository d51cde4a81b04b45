// Clustering on the GPU: single-linkage dereplication of a collection from the cells of its pair matrix (not in the reference,
// whose end product is the two n x n matrices).
//
// Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, a cell i << 48 | j << 32 | x_ij names the keys two
// sketches share.  i < j are linked iff x_ij >= 1 and x_ij * den >= num * (c_i + c_j - x_ij) (Jaccard) or x_ij * den >=
// num * min(c_i, c_j) (the larger containment): integers only.  A cluster is a connected component, numbered by its
// first-listed member; its representative is the member with the most keys, the first listed among equals.
//
// One fixed chain of launches whatever n and n_cells are:
//   k_cl_init     a lane per sketch: parent[i] = i, size / best / shared = 0; the counter words
//   k_cl_link     a lane per cell (tiles of 2048, grid-stride): range check, the threshold test, and for an edge a lock-free
//                 union -- both roots by path halving, then a 32-bit atomicCAS hooks the LARGER root under the smaller one and
//                 the lane goes on from the new roots when it lost.  A root only ever moves to a smaller index, so the root a
//                 component ends with is its first-listed member.  Edges are counted per wave (ballot + popcount) and added
//                 once per wave.  No workgroup waits for another one
//   k_cl_flatten  a lane per sketch: root[i] = find(i), size[root] += 1, best[root] = max(best[root], c_i << 16 | 0xFFFF - i):
//                 the tie rule is a property of the maximum
//   scan          launch_scan_u32 over the "is a root" flags: the cluster number in first-member order, and the cluster count
//   k_cl_shared   a second pass over the cells: a cell whose two ends are in one cluster and one of them is its representative
//                 is the other end's `shared` (each (member, representative) pair occurs at most once: a plain store)
//   k_cl_rows     a lane per sketch: the 24-byte row
// and ONE host wait, for the rows, the two counts and the bad-cell word.  The host never iterates to a fixed point.
//
// What the union relies on.  parent[x] <= x always and parent[x] == x only for a root, a value written to parent[x] is an
// ancestor x had at some time, and a node that has been hooked never becomes a root again.  A lane that reads an OLD parent word
// (another XCD's L2 line, say) therefore still walks down inside x's component towards smaller indices and ends; the only step
// that must see the truth is the hook, and that is an atomicCAS on the root's own word, which executes at the memory side.
#include <algorithm>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kClThreads = 256;                       // 4 waves
constexpr uint32_t kClTile = 2048;                         // cells per workgroup and turn: 8 rounds of 256
constexpr uint32_t kClBlocksPerCu = 8;
constexpr uint32_t kClMaxDen = 1000000u;
// A key count takes 48 bits of the `best` word (c << 16 | 0xFFFF - i) and must leave the word's top bit to the comparison: the
// counts a caller may pass are below 2^47.
constexpr int kClCardBits = 47;
// the counter words at the head of the work area
enum ClWord : uint32_t { kClwEdges = 0 /* u64: words 0-1 */, kClwBad = 2 /* u32 */, kClwWords = 4 };

// cl_load / cl_find / cl_union: spsp_device.h (the linkage tree hooks with the same three)

__global__ __launch_bounds__(256) void k_cl_init(uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ size,
                                                 unsigned long long* __restrict__ best, unsigned long long* __restrict__ shared,
                                                 uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < kClwWords) words[i] = 0u;
    if (i >= n) return;
    parent[i] = i; size[i] = 0u; best[i] = 0ull; shared[i] = 0ull;
}

// u_max = (2^64 - 1) / num: a right-hand side beyond 64 bits is larger than any left-hand side (count < 2^32, den <= 10^6:
// count * den < 2^52), so such a pair is not linked and the product is never formed.  With den <= 10^6 and counts below 2^40
// neither product can overflow at all: num * (c_i + c_j) < 2^20 * 2^41.
__global__ __launch_bounds__(kClThreads) void k_cl_link(const unsigned long long* __restrict__ cells, unsigned long long n_cells,
                                                        const unsigned long long* __restrict__ card, uint32_t n, uint32_t metric,
                                                        unsigned long long num, unsigned long long den, unsigned long long u_max,
                                                        uint32_t* __restrict__ parent, uint32_t* __restrict__ words) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long n_tiles = (n_cells + kClTile - 1) / kClTile;
    unsigned long long edges = 0;                          // of this wave (the same number in every lane)
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kClTile / kClThreads; ++r) {
            const unsigned long long e = tile * kClTile + r * kClThreads + threadIdx.x;
            bool edge = false;
            uint32_t i = 0, j = 0;
            if (e < n_cells) {
                const unsigned long long c = cells[e];
                i = (uint32_t)(c >> 48); j = (uint32_t)(c >> 32) & 0xffffu;
                const unsigned long long x = c & 0xffffffffull;
                if (i >= j || j >= n) atomicOr(words + kClwBad, 1u);   // (tested before the indices are used; the call is refused)
                else if (x) {
                    const unsigned long long ci = card[i], cj = card[j];
                    const unsigned long long u = metric == SPSP_CLUSTER_JACCARD ? ci + cj - x : (ci < cj ? ci : cj);
                    edge = u <= u_max && x * den >= num * u;
                }
            }
            edges += (unsigned long long)__popcll(__ballot(edge));   // (every lane of the wave is here)
            if (edge) cl_union(parent, i, j);
        }
    }
    if (lane == 0 && edges) atomicAdd(reinterpret_cast<unsigned long long*>(words + kClwEdges), edges);
}

__global__ __launch_bounds__(256) void k_cl_flatten(uint32_t n, const unsigned long long* __restrict__ card, uint32_t* __restrict__ parent,
                                                    uint32_t* __restrict__ root, uint32_t* __restrict__ size,
                                                    unsigned long long* __restrict__ best, uint32_t* __restrict__ is_root) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = cl_find(parent, i, cl_load(parent + i));   // (no union runs any more: the roots stand still)
    root[i] = r;
    is_root[i] = r == i ? 1u : 0u;
    atomicAdd(size + r, 1u);
    atomicMax(best + r, card[i] << 16 | (unsigned long long)(0xFFFFu - i));
}

__global__ __launch_bounds__(kClThreads) void k_cl_shared(const unsigned long long* __restrict__ cells, unsigned long long n_cells, uint32_t n,
                                                          const uint32_t* __restrict__ root, const unsigned long long* __restrict__ best,
                                                          unsigned long long* __restrict__ shared) {
    const unsigned long long n_tiles = (n_cells + kClTile - 1) / kClTile;
    for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll 1
        for (uint32_t r = 0; r < kClTile / kClThreads; ++r) {
            const unsigned long long e = tile * kClTile + r * kClThreads + threadIdx.x;
            if (e >= n_cells) continue;
            const unsigned long long c = cells[e];
            const uint32_t i = (uint32_t)(c >> 48), j = (uint32_t)(c >> 32) & 0xffffu;
            if (i >= j || j >= n) continue;                // (k_cl_link has raised the flag)
            const uint32_t ri = root[i];
            if (ri != root[j]) continue;
            const uint32_t rep = 0xFFFFu - (uint32_t)(best[ri] & 0xFFFFull);
            if (rep == i) shared[j] = c & 0xffffffffull;
            else if (rep == j) shared[i] = c & 0xffffffffull;
        }
    }
}

// number[r] for a root r = the roots in front of it
__global__ __launch_bounds__(256) void k_cl_rows(uint32_t n, const unsigned long long* __restrict__ card, const uint32_t* __restrict__ root,
                                                 const uint32_t* __restrict__ size, const unsigned long long* __restrict__ best,
                                                 const uint32_t* __restrict__ number, const unsigned long long* __restrict__ shared,
                                                 spsp_cluster_row* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root[i], rep = 0xFFFFu - (uint32_t)(best[r] & 0xFFFFull);
    spsp_cluster_row row;
    row.cluster = number[r]; row.representative = rep; row.size = size[r]; row.reserved = 0;
    row.shared = rep == i ? card[i] : shared[i];
    rows[i] = row;
}

}  // namespace

int cluster_check_args(uint32_t n, int metric, uint32_t num, uint32_t den) {
    if (n == 0 || n > 65535) { set_error("clustering takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (metric != SPSP_CLUSTER_JACCARD && metric != SPSP_CLUSTER_CONTAINMENT) { set_error("cluster metric %d: 0 (Jaccard) or 1 (containment)", metric); return SPSP_ERR_ARG; }
    if (num == 0 || num > den || den > kClMaxDen) { set_error("cluster threshold %u / %u: needs 1 <= num <= den <= %u", num, den, kClMaxDen); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

int cluster_cells_impl(spsp_ctx* ctx, const uint64_t* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric, uint32_t num,
                       uint32_t den, spsp_cluster_row* rows, uint64_t* n_clusters, uint64_t* n_edges) {
    int rc;
    if ((rc = cluster_check_args(n, metric, num, den))) return rc;
    if (n_cells && !d_cells) { set_error("NULL cell list"); return SPSP_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i)
        if (h_card[i] >> kClCardBits) { set_error("sketch %u has %llu keys: clustering takes key counts below 2^%d", i, (unsigned long long)h_card[i], kClCardBits); return SPSP_ERR_ARG; }
    // work area: counter words | card, best, shared (u64 x n) | parent, root, size (u32 x n) | is_root (u32 x (n + 1)) | number (u32 x (n + 2))
    const size_t n8 = (size_t)n * 8, n4 = ((size_t)n * 4 + 7) & ~(size_t)7;
    if ((rc = ctx->cl_work.reserve(64 + 3 * n8 + 5 * n4 + 64)) || (rc = ctx->cl_rows.reserve((size_t)n * sizeof(spsp_cluster_row)))) return rc;
    uint8_t* w = ctx->cl_work.as<uint8_t>();
    uint32_t* d_words = reinterpret_cast<uint32_t*>(w);
    unsigned long long* d_card = reinterpret_cast<unsigned long long*>(w + 64);
    unsigned long long *d_best = d_card + n, *d_shared = d_best + n;
    uint32_t* d_parent = reinterpret_cast<uint32_t*>(w + 64 + 3 * n8);
    uint32_t* d_root = reinterpret_cast<uint32_t*>(w + 64 + 3 * n8 + n4);
    uint32_t* d_size = reinterpret_cast<uint32_t*>(w + 64 + 3 * n8 + 2 * n4);
    uint32_t* d_isroot = reinterpret_cast<uint32_t*>(w + 64 + 3 * n8 + 3 * n4);
    uint32_t* d_number = reinterpret_cast<uint32_t*>(w + 64 + 3 * n8 + 4 * n4 + 8);
    spsp_cluster_row* d_rows = ctx->cl_rows.as<spsp_cluster_row>();
    const unsigned long long* cells = reinterpret_cast<const unsigned long long*>(d_cells);
    const uint32_t per_sketch = (n + 255) / 256;
    const uint64_t tiles = (n_cells + kClTile - 1) / kClTile;
    const uint32_t per_cell = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)std::max(ctx->n_cu, 1) * kClBlocksPerCu));
    SPSP_HIP(hipMemcpyAsync(d_card, h_card, n8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_cl_init, dim3(per_sketch), dim3(256), 0, ctx->stream, n, d_parent, d_size, d_best, d_shared, d_words);
    hipLaunchKernelGGL(k_cl_link, dim3(per_cell), dim3(kClThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, (const unsigned long long*)d_card, n,
                       (uint32_t)metric, (unsigned long long)num, (unsigned long long)den, ~0ull / num, d_parent, d_words);
    hipLaunchKernelGGL(k_cl_flatten, dim3(per_sketch), dim3(256), 0, ctx->stream, n, (const unsigned long long*)d_card, d_parent, d_root, d_size, d_best,
                       d_isroot);
    SPSP_HIP(hipGetLastError());
    if ((rc = launch_scan_u32(ctx, d_isroot, d_number, n, ctx->h_scalar + kHsClusterCount))) return rc;
    hipLaunchKernelGGL(k_cl_shared, dim3(per_cell), dim3(kClThreads), 0, ctx->stream, cells, (unsigned long long)n_cells, n, (const uint32_t*)d_root,
                       (const unsigned long long*)d_best, d_shared);
    hipLaunchKernelGGL(k_cl_rows, dim3(per_sketch), dim3(256), 0, ctx->stream, n, (const unsigned long long*)d_card, (const uint32_t*)d_root,
                       (const uint32_t*)d_size, (const unsigned long long*)d_best, (const uint32_t*)d_number, (const unsigned long long*)d_shared, d_rows);
    SPSP_HIP(hipGetLastError());
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsClusterEdges, d_words + kClwEdges, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsClusterBad, d_words + kClwBad, 4, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(rows, d_rows, (size_t)n * sizeof(spsp_cluster_row), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait (h_card has been read by then)
    if ((uint32_t)ctx->h_scalar[kHsClusterBad]) {
        set_error("a cell names a sketch outside the collection (or a pair that is not i < j)");
        memset(rows, 0, (size_t)n * sizeof(spsp_cluster_row));
        return SPSP_ERR_ARG;
    }
    *n_edges = ctx->h_scalar[kHsClusterEdges];
    *n_clusters = (uint32_t)ctx->h_scalar[kHsClusterCount];
    return SPSP_OK;
}

int cluster_payloads_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n, int metric, uint32_t num, uint32_t den,
                          const uint64_t* ds_threshold, uint32_t* k_out, uint32_t* m_out, uint64_t* card, std::vector<spsp_cluster_row>* rows,
                          uint64_t* n_clusters, uint64_t* n_edges) {
    rows->clear();
    *n_clusters = 0; *n_edges = 0;
    int rc;
    if ((rc = cluster_check_args(n, metric, num, den))) return rc;
    DecodedKeys keys;
    rc = decode_keys_impl(ctx, payloads, lens, n, nullptr, nullptr, ds_threshold, &keys, card);
    *k_out = keys.k; *m_out = keys.m;
    if (rc) return rc;
    uint64_t n_cells = 0;
    // the all-vs-all as cells for every n
    if (keys.sk_off[n] && n > 1 && (rc = compare_keys_cells(ctx, keys, n, n, &n_cells))) return rc;
    rows->resize(n);
    return cluster_cells_impl(ctx, ctx->m_cells.as<uint64_t>(), n_cells, card, n, metric, num, den, rows->data(), n_clusters, n_edges);
}

// spsp_cluster_files behind its argument checks: the sketches loaded (spsp_host.cpp), the clusters, <out_prefix>_clusters.csv.gz
static int cluster_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den, const char* out_prefix,
                         int chatter, double rate, std::vector<spsp_cluster_row>* rows, uint64_t* n_clusters) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "clustering is"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    uint32_t k = 0, m = 0;
    uint64_t n_edges = 0;
    std::vector<uint64_t>& card = run.card;
    rc = cluster_payloads_impl(ctx, run.L.data.data(), run.L.len.data(), n, metric, num, den, run.L.threshold(), &k, &m, card.data(), rows, n_clusters, &n_edges);
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_cluster_csv_host(rows->data(), paths, n, card.data(), metric, precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_clusters.csv.gz", t1)) || !chatter) return rc;
    uint32_t largest = 0;
    for (const spsp_cluster_row& r : *rows) largest = std::max(largest, r.size);
    printf("%u sketches, %llu edges, %llu clusters, the largest of %u\n", n, (unsigned long long)n_edges, (unsigned long long)*n_clusters, largest);
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_cluster_cells_device(spsp_ctx* ctx, const void* d_cells, uint64_t n_cells, const uint64_t* h_card, uint32_t n, int metric,
                                         uint32_t num, uint32_t den, spsp_cluster_row* rows, uint64_t* n_clusters, uint64_t* n_edges) {
    if (!ctx || !h_card || !rows || !n_clusters || !n_edges) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return cluster_cells_impl(ctx, (const uint64_t*)d_cells, n_cells, h_card, n, metric, num, den, rows, n_clusters, n_edges);
}

extern "C" int spsp_cluster_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, int precision, int metric, uint32_t num, uint32_t den,
                                  const char* out_prefix, int chatter, double rate, spsp_cluster_row** rows, uint64_t* n_clusters) {
    if (rows) *rows = nullptr;
    if (n_clusters) *n_clusters = 0;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = cluster_check_args(n, metric, num, den))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_cluster_row> got;
    uint64_t count = 0;
    if ((rc = cluster_files(ctx, paths, n, precision, metric, num, den, out_prefix, chatter, rate, &got, &count))) return rc;
    if (n_clusters) *n_clusters = count;
    return rows ? give_rows(got, rows) : SPSP_OK;
}
