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
//   flag, compact the downsampling unit's (ds_flag_compact_launch): k_ds_flag_band -- one workgroup per tile of 2048 entries: 4 B read
//                 per entry, the band test (merged: and the claimer's bit), a wave ballot -> k_ds_flag's keep mask and tile counts --
//                 then scan, k_ds_move, k_ds_offsets
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
    KeysShape shape;
    if ((rc = sorted_keys_front(ctx, "select reads", k, d_mn, d_lo, d_hi, h_sk_off, n, &shape))) return rc;
    const bool has_hi = shape.has_hi;
    const uint64_t first = shape.first, all_keys = shape.all_keys;
    const uint64_t sel_keys = h_sk_off[merged ? n : n_rows] - first;   // the entries that are asked: the rows', or (merged) everybody's
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
    // work area: flag words | the compaction's part
    const size_t words_bytes = 64;
    if ((rc = ctx->sel_work.reserve(words_bytes + DsWork::bytes(n_tiles, n_bounds)))) return rc;
    uint32_t* d_words = ctx->sel_work.as<uint32_t>();
    const DsWork W(ctx->sel_work.as<uint8_t>() + words_bytes, n_tiles, n_bounds);
    SPSP_HIP(hipMemsetAsync(d_words, 0, kSelWords * 4, ctx->stream));
    if ((rc = prevalence_fill_table(ctx, has_hi, d_mn, d_lo, d_hi, h_sk_off, n, nq, merged, d_words))) return rc;
    std::vector<uint64_t> rel(n_bounds);                            // (ours: the launcher's queued copy reads it, alive until the wait)
    ctx->h_scalar[kHsSelTotal] = 0;
    if (sel_keys) {
        for (uint32_t i = 0; i < n_bounds; ++i) rel[i] = merged ? (i ? sel_keys : 0) : h_sk_off[i] - first;
        if ((rc = ds_flag_compact_launch(ctx, W, has_hi, d_mn + first, d_lo + first, has_hi ? d_hi + first : nullptr, ctx->pv_hold.as<uint32_t>() + first,
                                         (uint32_t)sel_keys, h_min, h_max, merged ? 0x80000000u : 0u, rel.data(), n_bounds, o_mn, o_lo, o_hi,
                                         ctx->h_scalar + kHsSelTotal, sk_off_out))) return rc;
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

// (spsp_internal.h) the selected keys on the host: three copies and their wait
int fetch_keys(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, uint64_t total, HostKeys* keys) {
    keys->mn.resize(total); keys->lo.resize(total); keys->hi.resize(k > 32 ? total : 0);
    if (!total) return SPSP_OK;
    SPSP_HIP(hipMemcpyAsync(keys->mn.data(), d_mn, total * 4, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(keys->lo.data(), d_lo, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (k > 32) SPSP_HIP(hipMemcpyAsync(keys->hi.data(), d_hi, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));
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
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.load(rate);
    if (!rc) rc = run.refuse_k_eq_m(rc, "select is");
    double out_rate = run.L.ds_rate;
    if (!rc) rc = sketches_out_rate(run.L, paths, n, &out_rate);
    if ((rc = run.begin(rc))) return rc;
    const uint32_t R = n - n_query, n_out = each ? (n_query ? n_query : n) : 1u;
    std::vector<uint64_t> off(n_out + 1, 0);
    const DecodedKeys& keys = run.keys;
    uint32_t* d_mn = nullptr; uint64_t *d_lo = nullptr, *d_hi = nullptr;
    rc = run.decode();
    if (!rc) rc = keys_select_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), n, n_query, h_min, h_max, !each, &d_mn, &d_lo, &d_hi, off.data());
    const uint64_t total = off[n_out];
    HostKeys got;
    if (!rc) rc = fetch_keys(ctx, keys.k, d_mn, d_lo, d_hi, total, &got);
    ctx->stages.compare_s += now_s() - run.t0;                      // (booked in front of the writing; the payloads are released behind it)
    if (rc) return rc;
    uint64_t in = 0;
    for (uint32_t i = each ? 0 : n_query; i < (each ? n_out : n); ++i) in += run.card[i];
    const std::string list_path = std::string(out_prefix) + "_select.txt";
    const auto name_of = [&](uint32_t i) {
        if (!each) return std::string(out_prefix) + "_select.gz";
        const char* slash = strrchr(paths[i], '/');
        return std::string(out_prefix) + "_" + std::to_string(i) + "_" + (slash ? slash + 1 : paths[i]);
    };
    if ((rc = write_key_sketches(keys.k, keys.m, out_rate, got, off.data(), n_out, name_of, each ? list_path.c_str() : nullptr))) return rc;
    run.L.release();
    if (keys_in) *keys_in = in;
    if (keys_out) *keys_out = total;
    if (chatter) {
        if (h_min <= h_max) printf("%u reference(s), holder counts %u .. %u: %llu key(s) in, %llu written to %u sketch(es)\n", R, h_min, h_max,
                                   (unsigned long long)in, (unsigned long long)total, n_out);
        else printf("%u reference(s), an empty band of holder counts: %llu key(s) in, 0 written to %u sketch(es)\n", R, (unsigned long long)in, n_out);
        say_common_rate(run.L, n);
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
