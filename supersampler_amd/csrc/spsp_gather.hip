// Gather on the GPU: which references make up a query sketch, greedily (not in the reference, which stops at one row of
// containment numbers per query).
//
// Keys are the comparator's: the distinct (minimizer, canonical k-mer) pairs of a sketch, sorted by (minimizer, kmer_hi,
// kmer_lo).  Q = one query's keys, R_j = reference j's, A_0 = Q.  Round r: u_j = |R_j n A_{r-1}|; the winner j* is the
// SMALLEST j among the largest u_j; stop when u_j* < min_keys (or r > max_rounds); else emit (query, r, j*, |R_j* n Q|, u_j*,
// |A_{r-1}| - u_j*) and A_r = A_{r-1} \ R_j*.  Integers only.
//
// The work of all rounds together is bounded by one pass over the (reference key, query key) matches ("edges"):
//   k_g_match     a lane per reference key and query (grid.y): binary search in the query's sorted keys.  A match is appended
//                 to the edge list (one atomic per wave: ballot + prefix) and counted for its reference (u_j, which is also
//                 the `intersect` column) and for its query key (how many references hold it)
//   scan x 2      launch_scan_u32 over the per-reference and the per-query-key counts -> where each one's edges go
//   k_g_fill      a lane per edge: the edge's query key into its reference's list, its reference into its query key's list
//                 of holders (places by atomics: the order inside a list is arbitrary and nothing depends on it)
//   k_g_pick      one workgroup per query: arg-max over the u_j as (u << 32 | ~j) words, so the tie rule is a property of the
//                 maximum and not of the order lanes arrive in; lane 0 stops the query or writes the row and names the winner
//   k_g_walk      lanes over the winner's edges: a query key that is still alive dies, and every OTHER holder's counter goes
//                 down by one atomic.  The winner's keys are distinct, so a key dies once and the counters are exact.
// pick + walk are queued in batches of rounds; a stopped query's later launches return at their first load.  The host waits
// once for the edge count (it sizes the lists) and once per batch (rows, rows per query, stopped words).  No workgroup ever
// waits for another one: a round's order is the order of the launches on the stream.
#include <algorithm>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kGmThreads = 256;                       // 4 waves
constexpr uint32_t kGmTile = 2048;                         // reference keys per workgroup of k_g_match: 8 rounds of 256
constexpr uint32_t kGpThreads = 1024;                      // k_g_pick: one workgroup per query
constexpr uint32_t kGwThreads = 256;
constexpr uint32_t kGwMaxBlocks = 64;                      // k_g_walk: workgroups per query at the most
constexpr uint32_t kNoWinner = 0xffffffffu;
constexpr uint32_t kBatchFirst = 32, kBatchMax = 128;      // rounds queued per host wait: 32, 64, 128, 128, ...

// per-query words the round kernels keep (one host copy in, one per batch out)
struct GState { unsigned long long alive; uint32_t stopped, n_rows, winner, pad; };

template <bool HAS_HI>
__global__ __launch_bounds__(256) void k_g_check_queries(SortedKeys K, const uint64_t* __restrict__ off, uint32_t nq, uint32_t* __restrict__ flag) {
    const uint64_t e = off[0] + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= off[nq]) return;
    sorted_check_order<HAS_HI>(K, off, 0, nq, e, K.mn[e], HAS_HI ? K.hi[e] : 0ull, K.lo[e], flag);
}

// grid.x = tile of reference keys, grid.y = query.  edges[i] = reference (relative to nq) << 48 | query << 32 | query key
// (relative to off[0]); *n_edges counts every match, also those beyond `cap` (the host then makes room and runs this again).
template <bool HAS_HI>
__global__ __launch_bounds__(kGmThreads) void k_g_match(SortedKeys K, const uint64_t* __restrict__ off, uint32_t n, uint32_t nq,
                                                        unsigned long long* __restrict__ edges, unsigned long long cap,
                                                        unsigned long long* __restrict__ n_edges, uint32_t* __restrict__ u,
                                                        uint32_t* __restrict__ qcnt, uint32_t* __restrict__ flag) {
    const uint32_t q = blockIdx.y, nr = n - nq, lane = threadIdx.x & 63u;
    const uint64_t q_first = off[0], qs = off[q], qe = off[q + 1], r_first = off[nq], r_end = off[n];
    if (qs == qe && q != 0) return;                        // (uniform; query 0's workgroups also check the references' order)
#pragma unroll 1
    for (uint32_t r = 0; r < kGmTile / kGmThreads; ++r) {
        const uint64_t e = r_first + (uint64_t)blockIdx.x * kGmTile + r * kGmThreads + threadIdx.x;
        const bool valid = e < r_end;
        bool found = false;
        uint64_t at = 0;
        if (valid) {
            const uint32_t mn = K.mn[e];
            const uint64_t lo = K.lo[e], hi = HAS_HI ? K.hi[e] : 0ull;
            if (q == 0) sorted_check_order<HAS_HI>(K, off, nq, n, e, mn, hi, lo, flag);
            uint64_t a = qs, b = qe;                       // first query key that is not below this one
            while (a < b) { const uint64_t mid = a + ((b - a) >> 1); if (keys_less<HAS_HI>(K, mid, mn, hi, lo)) a = mid + 1; else b = mid; }
            at = a;
            found = a < qe && K.mn[a] == mn && K.lo[a] == lo && (!HAS_HI || K.hi[a] == hi);
        }
        const unsigned long long word = __ballot(found);   // (every lane of the wave is here: no lane has left the loop)
        if (word == 0ull) continue;
        unsigned long long base = 0;
        if (lane == (uint32_t)__ffsll((long long)word) - 1u) base = atomicAdd(n_edges, (unsigned long long)__popcll(word));
        base = __shfl(base, __ffsll((long long)word) - 1);
        if (!found) continue;
        const uint32_t jr = sorted_sketch_of(off, nq, n, e) - nq;
        const uint32_t qi = (uint32_t)(at - q_first);
        const unsigned long long pos = base + (unsigned long long)__popcll(word & ((1ull << lane) - 1ull));
        if (pos < cap) edges[pos] = (unsigned long long)jr << 48 | (unsigned long long)q << 32 | qi;
        atomicAdd(&u[(size_t)q * nr + jr], 1u);
        atomicAdd(&qcnt[qi], 1u);
    }
}

// r_off / q_off: the scans of u and of qcnt.  qcnt counts down to zero here: it is the rounds' `dead` array afterwards.
__global__ __launch_bounds__(256) void k_g_fill(const unsigned long long* __restrict__ edges, uint32_t n_edges, uint32_t nr,
                                                const uint32_t* __restrict__ r_off, uint32_t* __restrict__ r_fill, uint32_t* __restrict__ by_ref,
                                                const uint32_t* __restrict__ q_off, uint32_t* __restrict__ qcnt, uint32_t* __restrict__ holders) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_edges; i += gridDim.x * 256u) {
        const unsigned long long w = edges[i];
        const uint32_t jr = (uint32_t)(w >> 48), q = (uint32_t)(w >> 32) & 0xffffu, qi = (uint32_t)w;
        const size_t cell = (size_t)q * nr + jr;
        by_ref[r_off[cell] + atomicAdd(&r_fill[cell], 1u)] = qi;
        holders[q_off[qi] + atomicSub(&qcnt[qi], 1u) - 1u] = jr;
    }
}

// one workgroup per query; `slot`: this launch's place in the batch's rows (rows[q * batch + slot])
__global__ __launch_bounds__(kGpThreads) void k_g_pick(uint32_t* __restrict__ u, const uint32_t* __restrict__ r_off, uint32_t nq, uint32_t nr,
                                                       unsigned long long min_keys, uint32_t max_rounds, GState* __restrict__ state,
                                                       spsp_gather_row* __restrict__ rows, uint32_t batch, uint32_t slot) {
    __shared__ unsigned long long s_best[kGpThreads];
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    if (state[q].stopped) return;                          // (uniform: every lane reads the same word)
    const uint32_t* uq = u + (size_t)q * nr;
    unsigned long long best = 0;                           // value first, then the LOWEST index: u << 32 | ~j
    for (uint32_t j = t; j < nr; j += kGpThreads) {
        const unsigned long long w = (unsigned long long)uq[j] << 32 | (0xffffffffu - j);
        best = w > best ? w : best;
    }
    s_best[t] = best;
    __syncthreads();
#pragma unroll
    for (uint32_t d = kGpThreads / 2; d; d >>= 1) {
        if (t < d) { const unsigned long long o = s_best[t + d]; if (o > s_best[t]) s_best[t] = o; }
        __syncthreads();
    }
    if (t != 0) return;
    const unsigned long long top = s_best[0];
    const uint32_t best_u = (uint32_t)(top >> 32), j = 0xffffffffu - (uint32_t)top, rank = state[q].n_rows + 1;
    if ((unsigned long long)best_u < min_keys || (max_rounds && rank > max_rounds)) {
        state[q].stopped = 1u;
        state[q].winner = kNoWinner;
        return;
    }
    const size_t cell = (size_t)q * nr + j;
    const unsigned long long left = state[q].alive - best_u;
    spsp_gather_row row;
    row.query = q; row.rank = rank; row.match = nq + j; row.reserved = 0;
    row.intersect = r_off[cell + 1] - r_off[cell]; row.unique = best_u; row.remaining = left;
    rows[(size_t)q * batch + slot] = row;
    state[q].alive = left;
    state[q].n_rows = rank;
    state[q].winner = j;
    u[cell] = 0;                                           // all its keys die in this round: it is never named again
}

// grid.x = share of the winner's edges, grid.y = query
__global__ __launch_bounds__(kGwThreads) void k_g_walk(uint32_t* __restrict__ u, const uint32_t* __restrict__ r_off, const uint32_t* __restrict__ by_ref,
                                                       const uint32_t* __restrict__ q_off, const uint32_t* __restrict__ holders, uint32_t* __restrict__ dead,
                                                       uint32_t nr, const GState* __restrict__ state) {
    const uint32_t q = blockIdx.y, j = state[q].winner;
    if (j == kNoWinner) return;
    uint32_t* uq = u + (size_t)q * nr;
    const size_t cell = (size_t)q * nr + j;
    const uint32_t end = r_off[cell + 1];
    for (uint32_t i = r_off[cell] + blockIdx.x * kGwThreads + threadIdx.x; i < end; i += gridDim.x * kGwThreads) {
        const uint32_t qi = by_ref[i];                     // (the winner's keys are distinct: no other lane holds this one)
        if (dead[qi]) continue;
        dead[qi] = 1u;
        const uint32_t h_end = q_off[qi + 1];
        for (uint32_t h = q_off[qi]; h < h_end; ++h) { const uint32_t o = holders[h]; if (o != j) atomicSub(&uq[o], 1u); }
    }
}

}  // namespace

int gather_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                       uint32_t n, uint32_t nq, uint64_t min_keys, uint32_t max_rounds, std::vector<spsp_gather_row>* rows) {
    rows->clear();
    if (nq == 0 || nq >= n) { set_error("gather needs 1 <= n_query < n (n_query = %u, n = %u)", nq, n); return SPSP_ERR_ARG; }
    if (n > 65535) { set_error("gather takes at most 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (min_keys == 0) { set_error("min_keys must be >= 1"); return SPSP_ERR_ARG; }
    if (ctx->keys_unordered) { set_error("gather searches sorted sketches: not on a context switched to unordered keys"); return SPSP_ERR_ARG; }
    if (k < 1 || k > 63) { set_error("k=%u out of range 1..63", k); return SPSP_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i)
        if (h_sk_off[i + 1] < h_sk_off[i]) { set_error("sketch offsets must not decrease (sketch %u)", i); return SPSP_ERR_ARG; }
    const bool has_hi = k > 32;
    const uint32_t nr = n - nq;
    const uint64_t Qk = h_sk_off[nq] - h_sk_off[0], Rk = h_sk_off[n] - h_sk_off[nq], cells = (uint64_t)nq * nr;
    if (Qk > 0xfffffff0ull || Rk > 0xfffffff0ull) { set_error("too many sketch k-mers for one call"); return SPSP_ERR_OVERFLOW; }
    if (Qk == 0 || Rk == 0) return SPSP_OK;                // nothing can match: no rows
    if (!d_mn || !d_lo || (has_hi && !d_hi)) { set_error("NULL key array"); return SPSP_ERR_ARG; }
    const SortedKeys K{d_mn, d_lo, d_hi};
    int rc;
    // counters: [0] edges (64 bit), [2] order flag
    if ((rc = ctx->g_off.reserve(((size_t)n + 1) * 8)) || (rc = ctx->g_u.reserve((cells + 1) * 4)) || (rc = ctx->g_roff.reserve((cells + 1) * 4)) ||
        (rc = ctx->g_rfill.reserve(cells * 4)) || (rc = ctx->g_qcnt.reserve((Qk + 1) * 4)) || (rc = ctx->g_qoff.reserve((Qk + 1) * 4)) ||
        (rc = ctx->g_count.reserve(64)) || (rc = ctx->g_state.reserve((size_t)nq * sizeof(GState))) ||
        (rc = ctx->g_rows.reserve((size_t)nq * kBatchMax * sizeof(spsp_gather_row)))) return rc;
    uint64_t* d_off = ctx->g_off.as<uint64_t>();
    uint32_t *d_u = ctx->g_u.as<uint32_t>(), *d_roff = ctx->g_roff.as<uint32_t>(), *d_rfill = ctx->g_rfill.as<uint32_t>();
    uint32_t *d_qcnt = ctx->g_qcnt.as<uint32_t>(), *d_qoff = ctx->g_qoff.as<uint32_t>();
    unsigned long long* d_count = ctx->g_count.as<unsigned long long>();
    uint32_t* d_flag = reinterpret_cast<uint32_t*>(d_count + 2);
    SPSP_HIP(hipMemcpyAsync(d_off, h_sk_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t tiles = (uint32_t)((Rk + kGmTile - 1) / kGmTile);
    // room for the edges: what the last call on this context needed, at the least a quarter of the query keys per query
    uint64_t cap = std::max<uint64_t>(ctx->g_edges.cap / 8, std::max<uint64_t>(1u << 16, Qk / 4));
    uint64_t n_edges = 0;
    uint64_t h_count[3] = {0, 0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        if ((rc = ctx->g_edges.reserve((size_t)cap * 8))) return rc;
        SPSP_HIP(hipMemsetAsync(d_u, 0, (cells + 1) * 4, ctx->stream));
        SPSP_HIP(hipMemsetAsync(d_rfill, 0, cells * 4, ctx->stream));
        SPSP_HIP(hipMemsetAsync(d_qcnt, 0, (Qk + 1) * 4, ctx->stream));
        SPSP_HIP(hipMemsetAsync(d_count, 0, 24, ctx->stream));
        if (attempt == 0) {
            const uint32_t gx = (uint32_t)((Qk + 255) / 256);
            if (has_hi) hipLaunchKernelGGL(k_g_check_queries<true>, dim3(gx), dim3(256), 0, ctx->stream, K, (const uint64_t*)d_off, nq, d_flag);
            else hipLaunchKernelGGL(k_g_check_queries<false>, dim3(gx), dim3(256), 0, ctx->stream, K, (const uint64_t*)d_off, nq, d_flag);
        }
        if (has_hi) hipLaunchKernelGGL(k_g_match<true>, dim3(tiles, nq), dim3(kGmThreads), 0, ctx->stream, K, (const uint64_t*)d_off, n, nq,
                                       ctx->g_edges.as<unsigned long long>(), (unsigned long long)cap, d_count, d_u, d_qcnt, d_flag);
        else hipLaunchKernelGGL(k_g_match<false>, dim3(tiles, nq), dim3(kGmThreads), 0, ctx->stream, K, (const uint64_t*)d_off, n, nq,
                                ctx->g_edges.as<unsigned long long>(), (unsigned long long)cap, d_count, d_u, d_qcnt, d_flag);
        SPSP_HIP(hipGetLastError());
        SPSP_HIP(hipMemcpyAsync(h_count, d_count, 24, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // the wait that sizes the lists
        if (attempt == 0 && (uint32_t)h_count[2]) { set_error("sketch keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)"); return SPSP_ERR_ARG; }
        n_edges = h_count[0];
        if (n_edges > 0xfffffff0ull) { set_error("too many matches for one gather call (%llu)", (unsigned long long)n_edges); return SPSP_ERR_OVERFLOW; }
        if (n_edges <= cap) break;
        cap = n_edges;
    }
    if (n_edges == 0) return SPSP_OK;
    if ((rc = ctx->g_byref.reserve((size_t)n_edges * 4)) || (rc = ctx->g_hold.reserve((size_t)n_edges * 4))) return rc;
    if ((rc = launch_scan_u32(ctx, d_u, d_roff, cells, nullptr)) || (rc = launch_scan_u32(ctx, d_qcnt, d_qoff, Qk, nullptr))) return rc;
    hipLaunchKernelGGL(k_g_fill, dim3((uint32_t)std::min<uint64_t>(4096, (n_edges + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const unsigned long long*)ctx->g_edges.as<unsigned long long>(), (uint32_t)n_edges, nr, (const uint32_t*)d_roff, d_rfill,
                       ctx->g_byref.as<uint32_t>(), (const uint32_t*)d_qoff, d_qcnt, ctx->g_hold.as<uint32_t>());
    SPSP_HIP(hipGetLastError());
    std::vector<GState> st(nq);
    uint64_t max_ref = 0;
    for (uint32_t j = nq; j < n; ++j) max_ref = std::max(max_ref, h_sk_off[j + 1] - h_sk_off[j]);
    for (uint32_t q = 0; q < nq; ++q) { st[q].alive = h_sk_off[q + 1] - h_sk_off[q]; st[q].stopped = 0; st[q].n_rows = 0; st[q].winner = kNoWinner; st[q].pad = 0; }
    GState* d_state = ctx->g_state.as<GState>();
    spsp_gather_row* d_rows = ctx->g_rows.as<spsp_gather_row>();
    SPSP_HIP(hipMemcpyAsync(d_state, st.data(), (size_t)nq * sizeof(GState), hipMemcpyHostToDevice, ctx->stream));
    const uint32_t walk_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kGwMaxBlocks, (std::min(max_ref, n_edges) + kGwThreads - 1) / kGwThreads));
    std::vector<std::vector<spsp_gather_row>> per_query(nq);
    std::vector<spsp_gather_row> got;
    std::vector<uint32_t> had(nq, 0);
    uint32_t done = 0, batch = kBatchFirst;
    for (;;) {
        uint32_t B = batch;
        if (max_rounds) B = std::min(B, max_rounds - done);
        for (uint32_t s = 0; s < B; ++s) {
            hipLaunchKernelGGL(k_g_pick, dim3(nq), dim3(kGpThreads), 0, ctx->stream, d_u, (const uint32_t*)d_roff, nq, nr, (unsigned long long)min_keys,
                               max_rounds, d_state, d_rows, B, s);
            hipLaunchKernelGGL(k_g_walk, dim3(walk_blocks, nq), dim3(kGwThreads), 0, ctx->stream, d_u, (const uint32_t*)d_roff,
                               (const uint32_t*)ctx->g_byref.as<uint32_t>(), (const uint32_t*)d_qoff, (const uint32_t*)ctx->g_hold.as<uint32_t>(), d_qcnt,
                               nr, (const GState*)d_state);
        }
        SPSP_HIP(hipGetLastError());
        got.resize((size_t)nq * B);
        SPSP_HIP(hipMemcpyAsync(got.data(), d_rows, (size_t)nq * B * sizeof(spsp_gather_row), hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipMemcpyAsync(st.data(), d_state, (size_t)nq * sizeof(GState), hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // one wait per batch of rounds
        done += B;
        bool open = false;
        for (uint32_t q = 0; q < nq; ++q) {
            // a query's rows of this batch sit in its first slots: it is named in every launch until it stops, then never
            const uint32_t fresh = st[q].n_rows - had[q];
            per_query[q].insert(per_query[q].end(), got.begin() + (size_t)q * B, got.begin() + (size_t)q * B + fresh);
            had[q] = st[q].n_rows;
            if (!st[q].stopped) open = true;
        }
        if (!open || (max_rounds && done >= max_rounds)) break;
        batch = std::min(kBatchMax, batch * 2);
    }
    for (uint32_t q = 0; q < nq; ++q) rows->insert(rows->end(), per_query[q].begin(), per_query[q].end());
    return SPSP_OK;
}

int gather_payloads_impl(spsp_ctx* ctx, const uint8_t* const* payloads, const uint64_t* lens, uint32_t n, uint32_t n_query, uint64_t min_keys,
                         uint32_t max_rounds, const uint64_t* ds_threshold, uint32_t* k_out, uint32_t* m_out, uint64_t* card,
                         std::vector<spsp_gather_row>* rows) {
    rows->clear();
    DecodedKeys keys;
    const int rc = decode_keys_impl(ctx, payloads, lens, n, nullptr, nullptr, ds_threshold, &keys, card);
    *k_out = keys.k; *m_out = keys.m;
    if (rc || n == 0) return rc;
    return gather_device_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), n, n_query, min_keys, max_rounds, rows);
}

// spsp_gather_files behind its argument checks: the sketches loaded (spsp_host.cpp), the gather, <out_prefix>_gather.csv.gz
static int gather_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, uint64_t min_keys, uint32_t max_rounds,
                        const char* out_prefix, int chatter, double rate, std::vector<spsp_gather_row>* rows) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "gather is"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    uint32_t k = 0, m = 0;
    std::vector<uint64_t>& card = run.card;
    rc = gather_payloads_impl(ctx, run.L.data.data(), run.L.len.data(), n, n_query, min_keys, max_rounds, run.L.threshold(), &k, &m, card.data(), rows);
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_gather_csv_host(rows->data(), rows->size(), paths, n, n_query, card.data(), precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_gather.csv.gz", t1)) || !chatter) return rc;
    size_t at = 0;
    for (uint32_t q = 0; q < n_query; ++q) {
        uint64_t named = 0, left = card[q];
        for (; at < rows->size() && (*rows)[at].query == q; ++at) { ++named; left = (*rows)[at].remaining; }
        printf("%s: %llu reference(s) named, %llu of %llu keys remain\n", paths[q], (unsigned long long)named, (unsigned long long)left, (unsigned long long)card[q]);
    }
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_gather_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi,
                                  const uint64_t* h_sk_off, uint32_t n, uint32_t n_query, uint64_t min_keys, uint32_t max_rounds,
                                  spsp_gather_row* rows, uint64_t cap, uint64_t* n_rows) {
    if (!ctx || !h_sk_off || !n_rows || (cap && !rows)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_gather_row> out;
    const int rc = gather_device_impl(ctx, k, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n, n_query,
                                      min_keys, max_rounds, &out);
    if (rc) return rc;
    *n_rows = out.size();
    if (out.size() > cap) { set_error("%llu gather rows, room for %llu", (unsigned long long)out.size(), (unsigned long long)cap); return SPSP_ERR_OVERFLOW; }
    if (!out.empty()) memcpy(rows, out.data(), out.size() * sizeof(spsp_gather_row));
    return SPSP_OK;
}

extern "C" int spsp_gather_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, uint64_t min_keys,
                                 uint32_t max_rounds, const char* out_prefix, int chatter, double rate, spsp_gather_row** rows, uint64_t* n_rows) {
    if (rows) *rows = nullptr;
    if (n_rows) *n_rows = 0;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_query == 0 || n_query >= n) { set_error("gather needs 1 <= n_query < n (n_query = %u, n = %u)", n_query, n); return SPSP_ERR_ARG; }
    if (n > 65535) { set_error("gather takes at most 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (min_keys == 0) { set_error("min_keys must be >= 1"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_gather_row> got;
    const int rc = gather_files(ctx, paths, n, n_query, precision, min_keys, max_rounds, out_prefix, chatter, rate, &got);
    if (rc) return rc;
    if (n_rows) *n_rows = got.size();
    return rows ? give_rows(got, rows) : SPSP_OK;
}
