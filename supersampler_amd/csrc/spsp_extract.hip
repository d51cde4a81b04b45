// Extraction on the GPU: the records of a FASTA / FASTQ text that a record pass has called, written out again byte for byte (not
// in the reference, which has no record passes).  The rule is in include/spsp.h ("extract"); this file is its device form.
//
// Record starts (spsp_records_extents_device), laid out as the ingest: per 4 KiB tile a summary, one composing scan, one write.
//   k_ex_tail    one workgroup: is the text FASTQ (its first byte), where its content ends (behind the last byte that is neither
//                '\n' nor '\r': what fastq_tail finds on the host) and where its last record ends (behind the first '\n' of the
//                blank tail).  FASTA: both are n.  The words stay on the device: the launches behind it read them, no host wait.
//   k_ex_tiles   per tile: FASTA the lines behind byte 0 that begin with '>' or 0xFF; FASTQ the newlines of the content.
//   k_scan_items<ExSum>  one workgroup: the exclusive scan of the tiles' sums (spsp_device.h; it scans the records' sums below too).
//   k_ex_starts  per tile: begin[] -- FASTA every start; FASTQ the byte behind every newline whose line index is a multiple of
//                four ("line index mod 4 == 0" is decided here, behind the scan) -- and begin[n_rec], the last record's end.
// Kept lengths and output offsets: k_ex_rec_tiles / k_scan_items / k_ex_rec_write over tiles of 2 048 records.  A record adds its
// length when it is kept; consecutive kept records merge into RUNS (source start, output start), and the run table is what the
// copy searches: one entry per run, not per record.  Every pair begin[r] <= begin[r + 1] <= n is checked there (a d_begin of the
// caller's): a pair that fails adds nothing and raises the call's flag, so no run ever leaves the text.
// The copy (k_ex_copy), the hot path, is balanced by OUTPUT bytes: a workgroup owns a stretch of 16 KiB of the output, finds the
// runs that cross it with two binary searches, and every lane writes 16-byte-aligned 16-byte stores, each found by a search over
// the stretch's runs only.  A store inside one run takes two aligned 16-byte loads of the source and a byte shift; a store that
// straddles runs (or holds the appended newline, or the output's end) is assembled byte by byte.  The output buffer is whole
// stretches, as many as the grid has workgroups: no store can leave it whatever the table says.
// Ordering is by the launches on the stream; no device-wide atomics but the flag's; plain vector stores.
#include <algorithm>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kExChunk = 16;
static_assert(kExTile == kExThreads * kExChunk && kExStores * kExThreads * 16 == kExStretch, "the tile and the stretch in lanes");

// bit j: byte j of the 16 equals `byte` (four bytes per register: the exact zero-byte test, then the four flags of a word packed)
__device__ __forceinline__ uint32_t ex_eq16(const uint32_t (&w)[4], uint32_t byte) {
    uint32_t m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t x = w[d] ^ (byte * 0x01010101u);
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
        m |= ((((z >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * d);
    }
    return m;
}

// one lane's 16 bytes at p0.  nl: its newlines in front of `limit`; start (FASTA): the bytes behind byte 0 that begin a record
struct ExChunk { uint32_t nl, start; };
__device__ __forceinline__ ExChunk ex_chunk(const uint8_t* __restrict__ text, uint64_t n, uint64_t limit, uint64_t p0, bool fastq) {
    ExChunk c{0u, 0u};
    if (p0 >= n) return c;
    const uint32_t valid = n - p0 < (uint64_t)kExChunk ? (uint32_t)(n - p0) : kExChunk;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (valid == kExChunk) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kExChunk; ++j)
            if (j < valid) w[j >> 2] |= (uint32_t)text[p0 + j] << (8 * (j & 3));
    }
    const uint32_t in_mask = (1u << valid) - 1u;
    const uint32_t nl = ex_eq16(w, '\n') & in_mask;
    if (fastq) {
        c.nl = p0 >= limit ? 0u : (limit - p0 >= (uint64_t)kExChunk ? nl : nl & ((1u << (uint32_t)(limit - p0)) - 1u));
    } else {
        c.nl = nl;
        const uint32_t head = (ex_eq16(w, '>') | ex_eq16(w, 0xFFu)) & in_mask;
        uint32_t behind = nl << 1;                         // byte j sits behind a newline
        if ((head & 1u) && p0 > 0 && text[p0 - 1] == '\n') behind |= 1u;
        c.start = head & behind & 0xFFFFu;
    }
    return c;
}

__global__ __launch_bounds__(kExThreads) void k_ex_tail(const uint8_t* __restrict__ text, uint64_t n, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long s_best;
    const uint32_t t = threadIdx.x;
    const bool fastq = n > 0 && text[0] == '@';
    if (!fastq) {
        if (t == 0) { words[kExFastq] = 0ull; words[kExLimit] = n; words[kExEnd] = n; }
        return;
    }
    unsigned long long content_end = 0;
    for (uint64_t hi = n; hi > 0;) {                       // (uniform: byte 0 is '@', so the loop ends there at the latest)
        if (t == 0) s_best = 0ull;
        __syncthreads();
        const uint64_t lo = hi > kExThreads ? hi - kExThreads : 0, p = lo + t;
        if (p < hi && text[p] != '\n' && text[p] != '\r') atomicMax(&s_best, (unsigned long long)p + 1ull);
        __syncthreads();
        content_end = s_best;
        __syncthreads();
        if (content_end) break;
        hi = lo;
    }
    // the tail's first two newlines: the first ends the content's last line, the second an empty line behind it
    unsigned long long ends[2] = {content_end, n};         // (no newline: the last record lacks its own; the empty line runs to the text's end)
    uint64_t from = content_end;
    for (int which = 0; which < 2; ++which) {
        bool found = false;
        for (uint64_t lo = from; lo < n && !found; lo += kExThreads) {   // (uniform)
            if (t == 0) s_best = ~0ull;
            __syncthreads();
            const uint64_t p = lo + t;
            if (p < n && text[p] == '\n') atomicMin(&s_best, (unsigned long long)p);
            __syncthreads();
            const unsigned long long first = s_best;
            __syncthreads();
            if (first != ~0ull) { ends[which] = first + 1ull; found = true; }
        }
        if (!found) break;
        from = ends[which];
    }
    if (t == 0) {
        words[kExFastq] = 1ull; words[kExLimit] = content_end; words[kExEnd] = ends[0];
        words[kExBlank] = ends[0] > content_end && ends[0] < n ? 1ull : 0ull;
        words[kExEndEmpty] = ends[1];
    }
}

__global__ __launch_bounds__(kExThreads) void k_ex_tiles(const uint8_t* __restrict__ text, uint64_t n, const unsigned long long* __restrict__ words,
                                                         ExSum* __restrict__ tiles) {
    __shared__ uint32_t s_wave[kExThreads / 64];
    const bool fastq = words[kExFastq] != 0ull;
    const ExChunk c = ex_chunk(text, n, words[kExLimit], (uint64_t)blockIdx.x * kExTile + (uint64_t)threadIdx.x * kExChunk, fastq);
    const uint32_t total = block_sum<kExThreads / 64>((uint32_t)__popc(fastq ? c.nl : c.start), s_wave);
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = ExSum{total, 0u, 0u};
}

// what the item scan does with an ExSum total: totals[0] = all a, totals[1] = all b | all c << 32
struct ExTotals {
    unsigned long long* totals;
    __device__ void operator()(const ExSum& s) const { totals[0] = s.a; totals[1] = (unsigned long long)s.b | ((unsigned long long)s.c << 32); }
};

// begin[] has room for cap + 1 entries: nothing is written behind them, whatever the text holds
__global__ __launch_bounds__(kExThreads) void k_ex_starts(const uint8_t* __restrict__ text, uint64_t n, uint64_t n_tiles,
                                                          unsigned long long* __restrict__ words, const ExSum* __restrict__ base,
                                                          uint64_t* __restrict__ begin, uint32_t cap) {
    __shared__ uint32_t s_wave[kExThreads / 64];
    const bool fastq = words[kExFastq] != 0ull;
    const uint64_t limit = words[kExLimit];
    const uint64_t p0 = (uint64_t)blockIdx.x * kExTile + (uint64_t)threadIdx.x * kExChunk;
    const ExChunk c = ex_chunk(text, n, limit, p0, fastq);
    const uint32_t before = block_prefix_excl<kExThreads / 64>((uint32_t)__popc(fastq ? c.nl : c.start), threadIdx.x & 63u, threadIdx.x >> 6, s_wave);
    __syncthreads();
    if (blockIdx.x < n_tiles) {
        uint64_t g = base[blockIdx.x].a + before;          // FASTA: the starts, FASTQ: the newlines in front of this lane
        uint32_t rem = fastq ? c.nl : c.start;
        while (rem) {
            const uint32_t j = __ffs(rem) - 1;
            rem &= rem - 1;
            ++g;
            if (!fastq) { if (g <= cap) begin[g] = p0 + j; }   // (record g: record 0 begins at byte 0)
            else if ((g & 3ull) == 0ull && p0 + j + 1 < limit && (g >> 2) <= cap) begin[g >> 2] = p0 + j + 1;   // line g begins behind this newline
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t units = words[kExUnits];
        const bool empty_last = fastq && ((units + 1) & 3ull) == 3ull && words[kExBlank] != 0ull;   // (the ingest's empty read at the end)
        const uint64_t lines = units + 1 + (empty_last ? 1u : 0u);
        const uint64_t recs = fastq ? (limit ? lines >> 2 : 0ull) : units + 1;
        words[kExRecs] = recs;
        words[kExBad] = fastq && limit && (lines & 3ull) ? 1ull : 0ull;
        begin[0] = 0;
        if (recs <= cap) begin[recs] = words[empty_last ? kExEndEmpty : kExEnd];
    }
}

// the records r0 .. r0 + 7 of one lane: s = their kept bytes, runs and kept records; on_run(i, src, at): the lane's i-th run begins
// with source byte src, `at` kept bytes behind the lane's first.  A record is part of a run when it is kept and not empty
template <class OnRun>
__device__ __forceinline__ void ex_walk(const uint64_t* __restrict__ begin, const uint8_t* __restrict__ keep, uint32_t n_rec, uint64_t n_text, uint64_t r0,
                                        ExSum& s, bool& bad, OnRun on_run) {
    s = ExSum{0ull, 0u, 0u};
    bad = false;
    if (r0 >= n_rec) return;
    uint64_t b0 = begin[r0];
    bool prev = false;
    if (r0 > 0) { const uint64_t bp = begin[r0 - 1]; prev = keep[r0 - 1] != 0 && bp < b0 && b0 <= n_text; }
#pragma unroll
    for (uint32_t u = 0; u < kExRecsPerLane; ++u) {
        const uint64_t r = r0 + u;
        if (r >= n_rec) break;
        const uint64_t b1 = begin[r + 1];
        const bool ok = b0 <= b1 && b1 <= n_text;
        if (!ok) bad = true;
        const bool kf = keep[r] != 0, k = kf && ok && b1 > b0;
        if (k && !prev) { on_run(s.b, b0, s.a); ++s.b; }
        if (k) s.a += b1 - b0;
        s.c += kf;
        prev = k;
        b0 = b1;
    }
}

__global__ __launch_bounds__(kExThreads) void k_ex_rec_tiles(const uint64_t* __restrict__ begin, const uint8_t* __restrict__ keep, uint32_t n_rec,
                                                             uint64_t n_text, ExSum* __restrict__ tiles, unsigned long long* __restrict__ words) {
    __shared__ ExSum s_wave[kExThreads / 64];
    ExSum s;
    bool bad;
    ex_walk(begin, keep, n_rec, n_text, ((uint64_t)blockIdx.x * kExThreads + threadIdx.x) * kExRecsPerLane, s, bad, [](uint32_t, uint64_t, uint64_t) {});
    if (bad) atomicOr(words + kExBad, 2ull);
    const ExSum all = block_sum<kExThreads / 64>(s, s_wave);
    if (threadIdx.x == 0) tiles[blockIdx.x] = all;
}

// run i: source bytes [run_src[i], ...) -> output bytes [run_dst[i], run_dst[i + 1]); run_dst[n_runs] = the source bytes kept
__global__ __launch_bounds__(kExThreads) void k_ex_rec_write(const uint8_t* __restrict__ text, uint64_t n_text, const uint64_t* __restrict__ begin,
                                                             const uint8_t* __restrict__ keep, uint32_t n_rec, uint64_t n_tiles,
                                                             const ExSum* __restrict__ base, uint64_t* __restrict__ run_src, uint64_t* __restrict__ run_dst,
                                                             unsigned long long* __restrict__ words) {
    __shared__ Sum64x32 s_wave[kExThreads / 64];
    const uint64_t r0 = ((uint64_t)blockIdx.x * kExThreads + threadIdx.x) * kExRecsPerLane;
    ExSum s;
    bool bad;
    ex_walk(begin, keep, n_rec, n_text, r0, s, bad, [](uint32_t, uint64_t, uint64_t) {});
    const Sum64x32 before = block_prefix_excl<kExThreads / 64>(Sum64x32{s.a, s.b}, threadIdx.x & 63u, threadIdx.x >> 6, s_wave);
    if (blockIdx.x < n_tiles) {
        const unsigned long long a0 = base[blockIdx.x].a + before.a;
        const uint32_t b0 = base[blockIdx.x].b + before.b;
        ExSum again;
        ex_walk(begin, keep, n_rec, n_text, r0, again, bad, [=](uint32_t i, uint64_t src, uint64_t at) { run_src[b0 + i] = src; run_dst[b0 + i] = a0 + at; });
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t n_runs = (uint32_t)words[kExRunsKept];
        run_dst[n_runs] = words[kExSrc];
        unsigned long long nl = 0ull;
        if (n_rec) {                                       // only the text's last record can lack its newline
            const uint64_t b0 = begin[n_rec - 1], b1 = begin[n_rec];
            if (keep[n_rec - 1] && b0 < b1 && b1 <= n_text && text[b1 - 1] != '\n') nl = 1ull;
        }
        words[kExNl] = nl;
    }
}

__global__ __launch_bounds__(kExThreads) void k_ex_copy(const uint8_t* __restrict__ text, uint64_t n_text, const uint64_t* __restrict__ run_src,
                                                        const uint64_t* __restrict__ run_dst, const unsigned long long* __restrict__ words,
                                                        uint8_t* __restrict__ out) {
    __shared__ uint32_t s_range[2];
    const uint64_t n_src = words[kExSrc], n_out = n_src + words[kExNl];
    const uint32_t n_runs = (uint32_t)words[kExRunsKept];
    const uint64_t o_wg = (uint64_t)blockIdx.x * kExStretch;
    if (o_wg >= n_out || n_runs == 0u) return;             // (uniform.  The grid is sized by the text: the output may be far shorter)
    if (threadIdx.x == 0u) s_range[0] = ex_find(run_dst, 0u, n_runs, o_wg);
    if (threadIdx.x == 64u) s_range[1] = ex_find(run_dst, 0u, n_runs, (o_wg + kExStretch < n_out ? o_wg + kExStretch : n_out) - 1ull);
    __syncthreads();
    const uint32_t i_lo = s_range[0], i_hi = s_range[1] + 1u;
#pragma unroll
    for (uint32_t it = 0; it < kExStores; ++it) {
        const uint64_t o = o_wg + (uint64_t)(it * kExThreads + threadIdx.x) * 16ull;
        if (o >= n_out) break;
        uint32_t i = ex_find(run_dst, i_lo, i_hi, o);
        uint64_t rd = run_dst[i], re = run_dst[i + 1], rs = run_src[i];
        uint4 v;
        if (o + 16ull <= re) {
            // inside one run: the 16 source bytes, out of the two aligned groups that hold them
            v = ex_gather16(text, n_text, rs + (o - rd));
        } else {
            // across runs, the appended newline or the output's end: byte by byte (zeros behind the end: the buffer is whole stretches)
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t b = 0; b < 16u; ++b) {
                const uint64_t pos = o + b;
                uint32_t byte = 0u;
                if (pos < n_src) {
                    while (pos >= re) { ++i; rs = run_src[i]; rd = re; re = run_dst[i + 1]; }   // (runs are not empty and run_dst[n_runs] = n_src)
                    byte = text[rs + (pos - rd)];
                } else if (pos < n_out) byte = '\n';
                w[b >> 2] |= byte << (8 * (b & 3u));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(out + o) = v;
    }
}

int ex_mark(spsp_ctx* ctx, int i) {
    if (!ctx->timing) return SPSP_OK;
    if (!ctx->ex_ev[i]) SPSP_HIP(hipEventCreate(&ctx->ex_ev[i]));
    SPSP_HIP(hipEventRecord(ctx->ex_ev[i], ctx->stream));
    ctx->ex_marked |= 1u << i;
    return SPSP_OK;
}

}  // namespace

int ex_front(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t* n_tiles) {
    if (((uintptr_t)d_text & 15u) != 0) { set_error("d_text must be 16-byte aligned"); return SPSP_ERR_ARG; }
    *n_tiles = (n_text + kExTile - 1) / kExTile;
    if (*n_tiles > 0x7fffffffull) { set_error("text too large for one call"); return SPSP_ERR_OVERFLOW; }
    return SPSP_OK;
}

// the tail, the tiles' sums and their scan: everything of the extents pass that does not need n_rec
int ex_count_launch(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t n_tiles) {
    int rc;
    if ((rc = ctx->ex_words.reserve(kExWords * 8)) || (rc = ctx->ex_tiles.reserve((size_t)(n_tiles + 1) * sizeof(ExSum))) ||
        (rc = ctx->ex_bases.reserve((size_t)(n_tiles + 1) * sizeof(ExSum)))) return rc;
    unsigned long long* words = ctx->ex_words.as<unsigned long long>();
    SPSP_HIP(hipMemsetAsync(words, 0, kExWords * 8, ctx->stream));
    hipLaunchKernelGGL(k_ex_tail, dim3(1), dim3(kExThreads), 0, ctx->stream, d_text, n_text, words);
    if (n_tiles) hipLaunchKernelGGL(k_ex_tiles, dim3((uint32_t)n_tiles), dim3(kExThreads), 0, ctx->stream, d_text, n_text, (const unsigned long long*)words,
                                    ctx->ex_tiles.as<ExSum>());
    hipLaunchKernelGGL((k_scan_items<ExSum, ExTotals>), dim3(1), dim3(1024), 0, ctx->stream, (const ExSum*)ctx->ex_tiles.as<ExSum>(), n_tiles,
                       ctx->ex_bases.as<ExSum>(), ExTotals{words + kExUnits});
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

// begin[0 .. cap] in the context's buffer
int ex_starts_launch(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t n_tiles, uint32_t cap) {
    int rc;
    if ((rc = ctx->ex_begin.reserve(((size_t)cap + 1) * 8))) return rc;
    hipLaunchKernelGGL(k_ex_starts, dim3((uint32_t)std::max<uint64_t>(n_tiles, 1)), dim3(kExThreads), 0, ctx->stream, d_text, n_text, n_tiles,
                       ctx->ex_words.as<unsigned long long>(), (const ExSum*)ctx->ex_bases.as<ExSum>(), ctx->ex_begin.as<uint64_t>(), cap);
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

int ex_refuse_lines(uint64_t lines) {
    set_error("FASTQ: the content has %llu line(s), which is not a multiple of four", (unsigned long long)lines);
    return SPSP_ERR_FORMAT;
}

int ex_scan_launch(spsp_ctx* ctx, const ExSum* d_in, uint64_t n_items, ExSum* d_out, unsigned long long* d_totals) {
    hipLaunchKernelGGL((k_scan_items<ExSum, ExTotals>), dim3(1), dim3(1024), 0, ctx->stream, d_in, n_items, d_out, ExTotals{d_totals});
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

int records_extents_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t** d_begin, uint32_t* n_rec, bool* fastq) {
    int rc;
    uint64_t n_tiles = 0;
    if ((rc = ex_front(ctx, d_text, n_text, &n_tiles)) || (rc = ex_mark(ctx, 0)) || (rc = ex_count_launch(ctx, d_text, n_text, n_tiles))) return rc;
    uint64_t h[kExWords];
    SPSP_HIP(hipMemcpyAsync(h, ctx->ex_words.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the wait that learns n_rec
    const bool fq = h[kExFastq] != 0;
    const uint64_t lines = h[kExUnits] + 1 + (fq && ((h[kExUnits] + 1) & 3ull) == 3ull && h[kExBlank] ? 1u : 0u);   // (as k_ex_starts counts them)
    if (fq && h[kExLimit] && (lines & 3ull)) return ex_refuse_lines(h[kExUnits] + 1);
    const uint64_t recs = fq ? (h[kExLimit] ? lines >> 2 : 0ull) : h[kExUnits] + 1;
    if (recs > 0xfffffff0ull) { set_error("too many records for one call"); return SPSP_ERR_OVERFLOW; }
    if ((rc = ex_starts_launch(ctx, d_text, n_text, n_tiles, (uint32_t)recs)) || (rc = ex_mark(ctx, 1))) return rc;
    *d_begin = ctx->ex_begin.as<uint64_t>(); *n_rec = (uint32_t)recs;
    if (fastq) *fastq = fq;
    return SPSP_OK;
}

int records_extract_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_begin, uint32_t n_rec, const uint8_t* h_keep,
                         uint8_t** d_out, uint64_t* n_out, uint64_t* n_kept, bool* fastq) {
    int rc;
    *d_out = nullptr; *n_out = 0; *n_kept = 0;
    if (n_rec > 0xfffffff0u) { set_error("too many records for one call (%u)", n_rec); return SPSP_ERR_OVERFLOW; }
    uint64_t n_tiles = 0;
    if ((rc = ex_front(ctx, d_text, n_text, &n_tiles)) || (rc = ex_mark(ctx, 0))) return rc;
    const bool own = d_begin == nullptr;
    if (own) {
        if ((rc = ex_count_launch(ctx, d_text, n_text, n_tiles)) || (rc = ex_starts_launch(ctx, d_text, n_text, n_tiles, n_rec))) return rc;
        d_begin = ctx->ex_begin.as<uint64_t>();
    } else {
        if ((rc = ctx->ex_words.reserve(kExWords * 8))) return rc;
        SPSP_HIP(hipMemsetAsync(ctx->ex_words.p, 0, kExWords * 8, ctx->stream));
    }
    if ((rc = ex_mark(ctx, 1))) return rc;
    const uint64_t n_rtiles = ((uint64_t)n_rec + kExRecTile - 1) / kExRecTile;
    const uint64_t grid = (n_text + 1 + kExStretch - 1) / kExStretch;   // the output is the text and one newline at the most
    if (grid > 0x7fffffffull) { set_error("text too large for one call"); return SPSP_ERR_OVERFLOW; }
    if ((rc = ctx->ex_keep.reserve((size_t)n_rec + 64)) || (rc = ctx->ex_tiles.reserve((size_t)(n_rtiles + 1) * sizeof(ExSum))) ||
        (rc = ctx->ex_bases.reserve((size_t)(n_rtiles + 1) * sizeof(ExSum))) || (rc = ctx->ex_runs.reserve(((size_t)n_rec / 2 + 2) * 16 + 16)) ||
        (rc = ctx->ex_out.reserve((size_t)grid * kExStretch))) return rc;
    unsigned long long* words = ctx->ex_words.as<unsigned long long>();
    uint8_t* keep = ctx->ex_keep.as<uint8_t>();
    uint64_t* run_dst = ctx->ex_runs.as<uint64_t>();        // n_rec / 2 + 2 entries: kept and dropped records alternate at the worst
    uint64_t* run_src = run_dst + ((size_t)n_rec / 2 + 2);
    if (n_rec) SPSP_HIP(hipMemcpyAsync(keep, h_keep, n_rec, hipMemcpyHostToDevice, ctx->stream));
    if (n_rtiles) hipLaunchKernelGGL(k_ex_rec_tiles, dim3((uint32_t)n_rtiles), dim3(kExThreads), 0, ctx->stream, d_begin, (const uint8_t*)keep, n_rec, n_text,
                                     ctx->ex_tiles.as<ExSum>(), words);
    hipLaunchKernelGGL((k_scan_items<ExSum, ExTotals>), dim3(1), dim3(1024), 0, ctx->stream, (const ExSum*)ctx->ex_tiles.as<ExSum>(), n_rtiles,
                       ctx->ex_bases.as<ExSum>(), ExTotals{words + kExSrc});
    hipLaunchKernelGGL(k_ex_rec_write, dim3((uint32_t)std::max<uint64_t>(n_rtiles, 1)), dim3(kExThreads), 0, ctx->stream, d_text, n_text, d_begin,
                       (const uint8_t*)keep, n_rec, n_rtiles, (const ExSum*)ctx->ex_bases.as<ExSum>(), run_src, run_dst, words);
    SPSP_HIP(hipGetLastError());
    if ((rc = ex_mark(ctx, 2))) return rc;
    hipLaunchKernelGGL(k_ex_copy, dim3((uint32_t)grid), dim3(kExThreads), 0, ctx->stream, d_text, n_text, (const uint64_t*)run_src, (const uint64_t*)run_dst,
                       (const unsigned long long*)words, ctx->ex_out.as<uint8_t>());
    SPSP_HIP(hipGetLastError());
    if ((rc = ex_mark(ctx, 3))) return rc;
    uint64_t h[kExWords];
    SPSP_HIP(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the wait that learns n_out
    if (ctx->timing && (ctx->ex_marked & 15u) == 15u)
        for (int i = 0; i < 3; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ctx->ex_ev[i], ctx->ex_ev[i + 1])); ctx->ex_ms[i] += ms; }
    ctx->ex_marked = 0;
    if (own) {
        if (h[kExBad] & 1ull) return ex_refuse_lines(h[kExUnits] + 1);
        if (h[kExRecs] != n_rec) {
            set_error("extract: the text holds %llu record(s), the flags are for %u", (unsigned long long)h[kExRecs], n_rec);
            return SPSP_ERR_ARG;
        }
    }
    if (h[kExBad] & 2ull) { set_error("extract: d_begin must not decrease and must end inside the text"); return SPSP_ERR_ARG; }
    *d_out = ctx->ex_out.as<uint8_t>();
    *n_out = h[kExSrc] + h[kExNl];
    *n_kept = h[kExRunsKept] >> 32;
    if (fastq) *fastq = own ? h[kExFastq] != 0 : false;
    return SPSP_OK;
}

int ExtractRun::on_text(spsp_ctx* side, const uint8_t* d_text, uint64_t n_text, uint32_t n_records, const uint8_t* keep) {
    int rc;
    uint8_t* d_out = nullptr;
    uint64_t n_out = 0;
    // (the ingest has told the road n_records: the starts are made for as many, with no wait of their own)
    if ((rc = records_extract_impl(side, d_text, n_text, nullptr, n_records, keep, &d_out, &n_out, &n_kept, &fastq))) return rc;
    n_rec = n_records;
    out.resize((size_t)n_out);
    if (n_out) SPSP_HIP(hipMemcpyAsync(out.data(), d_out, (size_t)n_out, hipMemcpyDeviceToHost, side->stream));   // only the kept bytes come back
    SPSP_HIP(hipStreamSynchronize(side->stream));
    return SPSP_OK;
}

int ExtractRun::write(spsp_ctx* ctx, const char* out_prefix, int chatter) {
    const std::string path = std::string(out_prefix) + "_extract" + tag + (fastq ? ".fq" : ".fa") + (gz ? ".gz" : "");
    const double t = now_s();
    const int rc = write_bytes(path.c_str(), out.data(), out.size(), gz);
    ctx->stages.csv_gzip_s += now_s() - t;
    if (!rc && chatter) {
        printf("extract %s: %llu of %llu record(s) kept, %llu byte(s) written to %s\n", what, (unsigned long long)n_kept, (unsigned long long)n_rec,
               (unsigned long long)out.size(), path.c_str());
        fflush(stdout);
    }
    return rc;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_records_extents_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, void** d_begin, uint32_t* n_rec) {
    if (!ctx || !d_begin || !n_rec || (n_text && !d_text)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint64_t* b = nullptr;
    *d_begin = nullptr; *n_rec = 0;
    const int rc = records_extents_impl(ctx, (const uint8_t*)d_text, n_text, &b, n_rec, nullptr);
    ctx->ex_marked = 0;
    if (!rc) *d_begin = b;
    return rc;
}

extern "C" int spsp_records_extract_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, const void* d_begin, uint32_t n_rec, const uint8_t* h_keep,
                                           void** d_out, uint64_t* n_out, uint64_t* n_kept) {
    if (!ctx || !d_out || !n_out || !n_kept || (n_text && !d_text) || (n_rec && !h_keep)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint8_t* o = nullptr;
    const int rc = records_extract_impl(ctx, (const uint8_t*)d_text, n_text, (const uint64_t*)d_begin, n_rec, h_keep, &o, n_out, n_kept, nullptr);
    *d_out = o;
    return rc;
}

extern "C" int spsp_extract_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (int i = 0; i < 3; ++i) { ms[i] = ctx->ex_ms[i]; ctx->ex_ms[i] = 0; }
    return SPSP_OK;
}
