// Selection on the GPU: the keys of a collection whose holder count lies in a band, written out as sketches again (not in the
// reference, whose end product is the two n x n matrices).  What the prevalence pass counts -- the core, the shell, the unique keys
// of a collection -- leaves here as keys the comparator can read again; the union and the intersection are two more bands.
//
// Keys and notation are the prevalence pass's (spsp_prevalence.hip): sketches 0 .. n-1 back to back, each sorted by (minimizer,
// kmer_hi, kmer_lo); n_query == 0: every sketch is a row and a reference (R = n), else the first n_query are rows only;
// h(x) = the references that hold key x.  A key passes iff h_min <= h(x) <= h_max, and nothing else decides.
//   each    every row sketch keeps its passing keys in their old order: n_rows sketches back to back
//   merged  the distinct keys of the references' union that pass, strictly increasing: ONE sketch
//
// One chain of launches whatever the sketches are:
//   table fill    prevalence's own (prevalence_fill_table): memset, k_pv_count, k_pv_read -> holders[e] = h of entry e; for the
//                 merged form k_pv_read also sets bit 31 of the one entry per distinct key that claimed the key's slot
//   k_sel_flag    one workgroup per tile of 2048 entries: 4 B read per entry, the band test (merged: and the claimer's bit), a wave
//                 ballot -> k_ds_flag's keep mask and tile counts
//   compaction    the downsampling pass's (ds_compact_launch): scan, k_ds_move, k_ds_offsets
//   merged only   big_sort_segments over the compacted keys as one segment (entry order is sorted per sketch, not across them)
// Host waits: one for `each` (the offsets, with the order check); for merged that one (it sizes the sort) and the sort's own.
// No workgroup ever waits for another one.
#include <algorithm>
#include <cstring>
#include <string>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kSelWords = 4;                          // flag words in front of the work area: keys out of order | a probe went round | 2 spare

// keep bit of entry i of [0, n_keys): holders[i] in [h_min, h_max]; need = 0x80000000 for the merged form -- only the entry that
// claimed its key's slot speaks for the key -- else 0.  Round r of wave w of tile t fills word 32 t + 4 r + w (k_ds_flag's layout)
__global__ __launch_bounds__(kDsThreads) void k_sel_flag(const uint32_t* __restrict__ holders, uint32_t n_keys, uint32_t h_min, uint32_t h_max,
                                                         uint32_t need, unsigned long long* __restrict__ mask, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_cnt[kDsThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * kDsTile + threadIdx.x;       // (n_keys <= 0xfffffff0 and the last tile starts below it)
    uint32_t v[kDsTile / kDsThreads];
#pragma unroll
    for (uint32_t r = 0; r < kDsTile / kDsThreads; ++r) {
        const uint64_t i = (uint64_t)base + r * kDsThreads;
        v[r] = i < n_keys ? holders[i] : 0u;
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kDsTile / kDsThreads; ++r) {
        const uint64_t i = (uint64_t)base + r * kDsThreads;
        const uint32_t h = v[r] & 0x7fffffffu;
        const bool keep = i < n_keys && (v[r] & need) == need && h >= h_min && h <= h_max;
        const unsigned long long word = __ballot(keep);
        if (lane == 0) mask[(size_t)blockIdx.x * kDsWords + r * (kDsThreads / 64) + w] = word;
        cnt += (uint32_t)__popcll(word);
    }
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

int select_check_args(uint32_t n, uint32_t n_query, bool merged) {
    if (n == 0 || n > 65535) { set_error("select takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_query >= n) { set_error("select: %u queries of %u sketches (0: every sketch is a row and a reference; else at least one reference behind them)", n_query, n); return SPSP_ERR_ARG; }
    if (merged && n_query) { set_error("select: the merged form is the references' union: it takes no queries (n_query = %u)", n_query); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

}  // namespace

int keys_select_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n,
                     uint32_t nq, uint32_t h_min, uint32_t h_max, bool merged, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi, uint64_t* sk_off_out) {
    int rc;
    if ((rc = select_check_args(n, nq, merged))) return rc;
    const uint32_t n_rows = nq ? nq : n, n_out = merged ? 1u : n_rows;
    for (uint32_t i = 0; i <= n_out; ++i) sk_off_out[i] = 0;
    if (ctx->keys_unordered) { set_error("select reads sorted sketches: not on a context switched to unordered keys"); return SPSP_ERR_ARG; }
    if (k < 1 || k > 63) { set_error("k=%u out of range 1..63", k); return SPSP_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i)
        if (h_sk_off[i + 1] < h_sk_off[i]) { set_error("sketch offsets must not decrease (sketch %u)", i); return SPSP_ERR_ARG; }
    const bool has_hi = k > 32;
    const uint64_t first = h_sk_off[0], extent = h_sk_off[n], all_keys = extent - first;
    const uint64_t sel_keys = h_sk_off[merged ? n : n_rows] - first;   // the entries that are asked: the rows', or (merged) everybody's
    if (extent > 0xfffffff0ull) { set_error("too many sketch k-mers for one call"); return SPSP_ERR_OVERFLOW; }
    if (all_keys && (!d_mn || !d_lo || (has_hi && !d_hi))) { set_error("NULL key array"); return SPSP_ERR_ARG; }
    // two sets of output arrays, used in turn: the result of one call may be the input of the next
    const int set = ctx->sel_flip;
    ctx->sel_flip ^= 1;
    if ((rc = ctx->sel_mn[set].reserve((size_t)sel_keys * 4 + 64)) || (rc = ctx->sel_lo[set].reserve((size_t)sel_keys * 8 + 64)) ||
        (has_hi && (rc = ctx->sel_hi[set].reserve((size_t)sel_keys * 8 + 64)))) return rc;
    uint32_t* o_mn = ctx->sel_mn[set].as<uint32_t>();
    uint64_t *o_lo = ctx->sel_lo[set].as<uint64_t>(), *o_hi = has_hi ? ctx->sel_hi[set].as<uint64_t>() : nullptr;
    *out_mn = o_mn; *out_lo = o_lo; *out_hi = o_hi;
    if (all_keys == 0) return SPSP_OK;
    const uint32_t n_tiles = (uint32_t)((sel_keys + kDsTile - 1) / kDsTile), n_bounds = n_out + 1;
    // work area: flag words | keep mask | offsets in | offsets out | tile counts | tile offsets (+ the total)
    const size_t words_bytes = 64, mask_bytes = (size_t)n_tiles * kDsWords * 8, off_bytes = (size_t)n_bounds * 8;
    if ((rc = ctx->sel_work.reserve(words_bytes + mask_bytes + 2 * off_bytes + ((size_t)2 * n_tiles + 2) * 4 + 64))) return rc;
    uint32_t* d_words = ctx->sel_work.as<uint32_t>();
    unsigned long long* d_mask = reinterpret_cast<unsigned long long*>(ctx->sel_work.as<uint8_t>() + words_bytes);
    uint64_t* d_off_in = reinterpret_cast<uint64_t*>(ctx->sel_work.as<uint8_t>() + words_bytes + mask_bytes);
    uint64_t* d_off_out = d_off_in + n_bounds;
    uint32_t* d_tile_cnt = reinterpret_cast<uint32_t*>(d_off_out + n_bounds);
    uint32_t* d_tile_off = d_tile_cnt + n_tiles;
    SPSP_HIP(hipMemsetAsync(d_words, 0, kSelWords * 4, ctx->stream));
    if ((rc = prevalence_fill_table(ctx, has_hi, d_mn, d_lo, d_hi, h_sk_off, n, nq, merged, d_words))) return rc;
    std::vector<uint64_t> rel(n_bounds);                            // (read by the copy below: alive until the wait)
    ctx->h_scalar[kHsSelTotal] = 0;
    if (sel_keys) {
        for (uint32_t i = 0; i < n_bounds; ++i) rel[i] = merged ? (i ? sel_keys : 0) : h_sk_off[i] - first;
        SPSP_HIP(hipMemcpyAsync(d_off_in, rel.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_sel_flag, dim3(n_tiles), dim3(kDsThreads), 0, ctx->stream, (const uint32_t*)(ctx->pv_hold.as<uint32_t>() + first), (uint32_t)sel_keys,
                           h_min, h_max, merged ? 0x80000000u : 0u, d_mask, d_tile_cnt);
        SPSP_HIP(hipGetLastError());
        if ((rc = ds_compact_launch(ctx, has_hi, d_mn + first, d_lo + first, has_hi ? d_hi + first : nullptr, d_mask, d_tile_cnt, d_tile_off, n_tiles, d_off_in,
                                    n_bounds, d_off_out, o_mn, o_lo, o_hi, ctx->h_scalar + kHsSelTotal))) return rc;
        SPSP_HIP(hipMemcpyAsync(sk_off_out, d_off_out, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsSelBad, d_words, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));                    // the wait: the offsets, the order check, (merged) the count
    if (ctx->h_scalar[kHsSelBad]) {
        set_error("sketch keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)");
        for (uint32_t i = 0; i <= n_out; ++i) sk_off_out[i] = 0;
        return SPSP_ERR_ARG;
    }
    if (!merged) return SPSP_OK;
    // entry order is sorted inside a sketch and not across them: the claimers of the union, as one segment, through the sort the
    // big genomes' keys take (chunks of 2048 in LDS, then merge passes); the other set's arrays are not touched -- they may be the input
    const uint64_t count = sk_off_out[1];
    if (count > 1) {
        if ((rc = ctx->sel_t_mn.reserve((size_t)count * 4 + 64)) || (rc = ctx->sel_t_lo.reserve((size_t)count * 8 + 64)) ||
            (has_hi && (rc = ctx->sel_t_hi.reserve((size_t)count * 8 + 64)))) { sk_off_out[1] = 0; return rc; }
        const std::vector<std::pair<uint32_t, uint32_t>> segs{{0u, (uint32_t)count}};
        if ((rc = big_sort_segments(ctx, has_hi, o_mn, o_lo, o_hi, ctx->sel_t_mn.as<uint32_t>(), ctx->sel_t_lo.as<uint64_t>(),
                                    has_hi ? ctx->sel_t_hi.as<uint64_t>() : nullptr, segs))) { sk_off_out[1] = 0; return rc; }
    }
    return SPSP_OK;
}

// (spsp_internal.h) the rate the output names: the common one where one was asked for, else the headers' if they all stand for one threshold
int sketches_out_rate(const LoadedSketches& L, const char* const* paths, uint32_t n, double* out_rate) {
    *out_rate = L.ds_rate;
    if (L.rate_asked) return SPSP_OK;
    uint64_t thr0 = 0; double last = 0; uint64_t last_thr = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t ki = 0, mi = 0; uint64_t cnt = 0; double ri = 0;
        const int rc = spsp_sketch_header_host(L.data[i], L.len[i], &ki, &mi, &cnt, &ri);
        if (rc) { const std::string why = spsp_last_error(); set_error("'%s': %s", paths[i], why.c_str()); return rc; }
        if (i == 0 || ri != last) { last = ri; last_thr = spsp_threshold_host(L.k, L.m, ri); }   // (powl once per run of equal rates)
        if (i == 0) { thr0 = last_thr; *out_rate = ri; }
        else if (last_thr != thr0) { set_error("sketches of different rates: give a rate ('%s' was sketched at rate %g, '%s' at %g)", paths[0], *out_rate, paths[i], ri); return SPSP_ERR_ARG; }
    }
    return SPSP_OK;
}

// spsp_select_files behind its argument checks: the sketches loaded (spsp_host.cpp), decoded (and brought down to the common
// rate), the selection, the selected keys copied back, one sketch file per output sketch (spsp_sketch_from_keys_host, gzip level 9
// as the sketcher writes) and, for `each`, the list of them
static int select_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, uint32_t h_min, uint32_t h_max, bool each,
                        const char* out_prefix, int chatter, double rate, uint64_t* keys_in, uint64_t* keys_out) {
    LoadedSketches L;
    int rc = load_sketch_files(ctx, paths, n, rate, &L);
    if (!rc && L.k && L.k == L.m) { set_error("select is not defined for k == m sketches (k = m = %u)", L.k); rc = SPSP_ERR_ARG; }
    double out_rate = L.ds_rate;
    if (!rc) rc = sketches_out_rate(L, paths, n, &out_rate);
    if (rc) { ctx->stages.compare_s += now_s() - L.t0; return rc; }
    const double t0 = files_loaded(ctx, L, n, chatter);
    const uint32_t R = n - n_query, n_out = each ? (n_query ? n_query : n) : 1u;
    std::vector<uint64_t> card(n, 0), off(n_out + 1, 0);
    DecodedKeys keys;
    uint32_t* d_mn = nullptr; uint64_t *d_lo = nullptr, *d_hi = nullptr;
    rc = decode_keys_impl(ctx, L.data.data(), L.len.data(), n, nullptr, nullptr, L.threshold(), &keys, card.data());
    if (!rc) rc = keys_select_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), n, n_query, h_min, h_max, !each, &d_mn, &d_lo, &d_hi, off.data());
    const uint32_t k = keys.k, m = keys.m;
    const uint64_t total = off[n_out];
    std::vector<uint32_t> mn(total);
    std::vector<uint64_t> lo(total), hi(k > 32 ? total : 0);
    if (!rc && total) {
        SPSP_HIP(hipMemcpyAsync(mn.data(), d_mn, total * 4, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipMemcpyAsync(lo.data(), d_lo, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (k > 32) SPSP_HIP(hipMemcpyAsync(hi.data(), d_hi, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->stages.compare_s += now_s() - t0;
    if (rc) return rc;
    uint64_t in = 0;
    for (uint32_t i = each ? 0 : n_query; i < (each ? n_out : n); ++i) in += card[i];
    std::string list;
    for (uint32_t i = 0; i < n_out; ++i) {
        std::string path = out_prefix;
        if (each) {
            const char* slash = strrchr(paths[i], '/');
            path += "_" + std::to_string(i) + "_" + (slash ? slash + 1 : paths[i]);
            list += path + "\n";
        } else path += "_select.gz";
        uint8_t* payload = nullptr; uint64_t len = 0;
        const uint64_t a = off[i], c = off[i + 1] - off[i];
        if ((rc = spsp_sketch_from_keys_host(k, m, out_rate, mn.data() + a, lo.data() + a, k > 32 ? hi.data() + a : nullptr, c, &payload, &len))) return rc;
        rc = spsp_write_gz_host(path.c_str(), payload, len, 9);
        free(payload);
        if (rc) return rc;
    }
    L.release();
    if (each) {
        const std::string path = std::string(out_prefix) + "_select.txt";
        FILE* f = fopen(path.c_str(), "wb");
        if (!f || fwrite(list.data(), 1, list.size(), f) != list.size() || fclose(f) != 0) { set_error("cannot write '%s'", path.c_str()); return SPSP_ERR_IO; }
    }
    if (keys_in) *keys_in = in;
    if (keys_out) *keys_out = total;
    if (chatter) {
        if (h_min <= h_max) printf("%u reference(s), holder counts %u .. %u: %llu key(s) in, %llu written to %u sketch(es)\n", R, h_min, h_max,
                                   (unsigned long long)in, (unsigned long long)total, n_out);
        else printf("%u reference(s), an empty band of holder counts: %llu key(s) in, 0 written to %u sketch(es)\n", R, (unsigned long long)in, n_out);
        say_common_rate(L, n);
        fflush(stdout);
    }
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_keys_select_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi,
                                       const uint64_t* h_sk_off, uint32_t n, uint32_t n_query, uint32_t h_min, uint32_t h_max, int merged,
                                       void** d_out_minimizer, void** d_out_kmer_lo, void** d_out_kmer_hi, uint64_t* sk_off_out) {
    if (!ctx || !h_sk_off || !d_out_minimizer || !d_out_kmer_lo || !d_out_kmer_hi || !sk_off_out) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    *d_out_minimizer = *d_out_kmer_lo = *d_out_kmer_hi = nullptr;
    SPSP_HIP(hipSetDevice(ctx->device));
    uint32_t* mn = nullptr; uint64_t *lo = nullptr, *hi = nullptr;
    const int rc = keys_select_impl(ctx, k, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n, n_query, h_min,
                                    h_max, merged != 0, &mn, &lo, &hi, sk_off_out);
    if (rc) return rc;
    *d_out_minimizer = mn; *d_out_kmer_lo = lo; *d_out_kmer_hi = hi;
    return SPSP_OK;
}

extern "C" int spsp_select_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, const char* what, int each,
                                 const char* out_prefix, int chatter, double rate, uint64_t* keys_in, uint64_t* keys_out) {
    if (keys_in) *keys_in = 0;
    if (keys_out) *keys_out = 0;
    if (!ctx || !paths || !what || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = select_check_args(n, n_query, !each))) return rc;
    uint32_t h_min = 1, h_max = 0;
    if ((rc = spsp_select_band_host(what, n - n_query, &h_min, &h_max))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    return select_files(ctx, paths, n, n_query, h_min, h_max, each != 0, out_prefix, chatter, rate, keys_in, keys_out);
}
