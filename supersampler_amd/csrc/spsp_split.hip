// Split on the GPU: every record of a FASTA / FASTQ text written to the slice of its bin, all bins in one pass over the text (not in
// the reference, which has no record passes).  The rule is in include/spsp.h ("split"); this file is its device form.  It is the
// extraction (spsp_extract.hip) with an ordering step between the run table and the copy:
//   starts    the extraction's own launches (ex_count_launch, ex_starts_launch), or the caller's begin[].
//   runs      k_sp_rec_tiles / the extraction's scan / k_sp_rec_write over tiles of 2 048 records: consecutive records of one bin
//             (not DROP, not empty) merge into a run.  Per run, in record order: its source start, the kept bytes in front of it
//             (pre[], so that a run's length is pre[i + 1] - pre[i]) and the sort's pair (key = bin, value = run number).
//             begin[] is checked as the extraction checks it: a pair that fails adds nothing and raises the call's flag.
//   order     radix_sort_pairs (spsp_build.hip), stable, over as many 8-bit digits as n_bins - 1 has.  The host counts the runs
//             the bins allow before anything is launched (the device cannot find more in a text whose records are not empty);
//             that count sizes the sort, and the places behind the runs the device did find hold keys of all ones, which a stable
//             sort leaves behind every run.  Runs are sorted, not records: labels that come in blocks sort in a few tiles.
//   offsets   k_sp_len_tiles / the scan / k_sp_dst_write over tiles of 2 048 sorted runs: run_dst[] by a 64-bit exclusive scan of
//             the sorted runs' lengths, the run of the text's last record one byte longer where that record lacks its newline; the
//             newline's output byte is a word of the call.  k_sp_bin_off: a lane per bin, one binary search over the sorted keys.
//   copy      k_sp_copy, the hot path: the extraction's schedule -- a workgroup owns kExStretch bytes of the output and finds the
//             runs that cross it by two binary searches over run_dst[]; a lane's aligned 16-byte store inside one run is two
//             aligned loads and a byte shift (ex_gather16), and only a store that crosses runs, holds the newline's byte or the
//             output's end is made byte by byte.  run_src[] is in no order here and nothing assumes one.
// A call whose flag is raised copies nothing: every kernel behind the run table reads the flag first.  The output buffer is whole
// stretches, as many as the copy's grid has workgroups.  Ordering is by the launches on the stream; no device-wide atomics but the
// flag's; plain vector stores.
#include <algorithm>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kSpDrop = SPSP_SPLIT_DROP;

// the records r0 .. r0 + 7 of one lane: s = their kept bytes and runs (c: the records with a bin); on_run(i, src, at, bin): the
// lane's i-th run begins with source byte src, `at` kept bytes behind the lane's first.  A record is part of a run when it has a
// bin and is not empty; it goes on the run of the record in front of it when that one is part of a run of the same bin
template <class OnRun>
__device__ __forceinline__ void sp_walk(const uint64_t* __restrict__ begin, const uint32_t* __restrict__ bin, uint32_t n_rec, uint64_t n_text, uint64_t r0,
                                        ExSum& s, bool& bad, OnRun on_run) {
    s = ExSum{0ull, 0u, 0u};
    bad = false;
    if (r0 >= n_rec) return;
    uint64_t b0 = begin[r0];
    uint32_t prev = kSpDrop;                               // the bin of the run the record in front belongs to
    if (r0 > 0) { const uint64_t bp = begin[r0 - 1]; if (bp < b0 && b0 <= n_text) prev = bin[r0 - 1]; }
#pragma unroll
    for (uint32_t u = 0; u < kExRecsPerLane; ++u) {
        const uint64_t r = r0 + u;
        if (r >= n_rec) break;
        const uint64_t b1 = begin[r + 1];
        const bool ok = b0 <= b1 && b1 <= n_text;
        if (!ok) bad = true;
        const uint32_t bn = bin[r];
        const bool k = bn != kSpDrop && ok && b1 > b0;
        if (k && bn != prev) { on_run(s.b, b0, s.a, bn); ++s.b; }
        if (k) s.a += b1 - b0;
        s.c += bn != kSpDrop;
        prev = k ? bn : kSpDrop;
        b0 = b1;
    }
}

__global__ __launch_bounds__(kExThreads) void k_sp_rec_tiles(const uint64_t* __restrict__ begin, const uint32_t* __restrict__ bin, uint32_t n_rec, uint64_t n_text,
                                                             ExSum* __restrict__ tiles, unsigned long long* __restrict__ words) {
    __shared__ ExSum s_wave[kExThreads / 64];
    ExSum s;
    bool bad;
    sp_walk(begin, bin, n_rec, n_text, ((uint64_t)blockIdx.x * kExThreads + threadIdx.x) * kExRecsPerLane, s, bad, [](uint32_t, uint64_t, uint64_t, uint32_t) {});
    if (bad) atomicOr(words + kExBad, 2ull);
    const ExSum all = block_sum<kExThreads / 64>(s, s_wave);
    if (threadIdx.x == 0) tiles[blockIdx.x] = all;
}

// run i, in record order: source bytes [src[i], src[i] + pre[i + 1] - pre[i]), keys[i] = its bin, vals[i] = i; pre[n_runs] = the
// source bytes kept.  The tables have room for `cap` runs: a run beyond them is not written, and the flag is raised
__global__ __launch_bounds__(kExThreads) void k_sp_rec_write(const uint8_t* __restrict__ text, uint64_t n_text, const uint64_t* __restrict__ begin,
                                                             const uint32_t* __restrict__ bin, uint32_t n_rec, uint64_t n_tiles, const ExSum* __restrict__ base,
                                                             uint32_t cap, uint64_t* __restrict__ src, uint64_t* __restrict__ pre, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ vals, unsigned long long* __restrict__ words) {
    __shared__ Sum64x32 s_wave[kExThreads / 64];
    const uint64_t r0 = ((uint64_t)blockIdx.x * kExThreads + threadIdx.x) * kExRecsPerLane;
    ExSum s;
    bool bad;
    sp_walk(begin, bin, n_rec, n_text, r0, s, bad, [](uint32_t, uint64_t, uint64_t, uint32_t) {});
    const Sum64x32 before = block_prefix_excl<kExThreads / 64>(Sum64x32{s.a, s.b}, threadIdx.x & 63u, threadIdx.x >> 6, s_wave);
    if (blockIdx.x < n_tiles) {
        const unsigned long long a0 = base[blockIdx.x].a + before.a;
        const uint32_t b0 = base[blockIdx.x].b + before.b;
        ExSum again;
        sp_walk(begin, bin, n_rec, n_text, r0, again, bad, [=](uint32_t i, uint64_t from, uint64_t at, uint32_t bn) {
            const uint32_t run = b0 + i;
            if (run < cap) { src[run] = from; pre[run] = a0 + at; keys[run] = bn; vals[run] = run; }
        });
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t n_runs = (uint32_t)words[kExRunsKept];
        if (n_runs > cap) atomicOr(words + kExBad, 4ull);
        else pre[n_runs] = words[kExSrc];
        unsigned long long nl = 0ull;
        if (n_rec) {                                       // only the text's last record can lack its newline
            const uint64_t e0 = begin[n_rec - 1], e1 = begin[n_rec];
            if (bin[n_rec - 1] != kSpDrop && e0 < e1 && e1 <= n_text && text[e1 - 1] != '\n') nl = 1ull;
        }
        words[kExNl] = nl;
        words[kSpNlAt] = ~0ull;
    }
}

// the runs the kernels behind the run table work on: none when the call's flag is raised
__device__ __forceinline__ uint32_t sp_live_runs(const unsigned long long* __restrict__ words, uint32_t cap) {
    if (words[kExBad] != 0ull) return 0u;
    const uint32_t n = (uint32_t)words[kExRunsKept];
    return n < cap ? n : cap;
}

// the output lengths of the sorted runs j0 .. j0 + 7 of one lane, and their sum.  The text's last record ends the last run in
// record order: that run counts the appended newline
__device__ __forceinline__ unsigned long long sp_lens(const uint32_t* __restrict__ vals, const uint64_t* __restrict__ pre, uint32_t n_runs, unsigned long long nl,
                                                      uint64_t j0, unsigned long long (&len)[kExRecsPerLane]) {
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t u = 0; u < kExRecsPerLane; ++u) {
        unsigned long long l = 0;
        if (j0 + u < n_runs) {
            const uint32_t v = vals[j0 + u];
            if (v < n_runs) l = pre[v + 1] - pre[v] + (v + 1u == n_runs ? nl : 0ull);
        }
        len[u] = l;
        sum += l;
    }
    return sum;
}

__global__ __launch_bounds__(kExThreads) void k_sp_len_tiles(const uint32_t* __restrict__ vals, const uint64_t* __restrict__ pre, uint32_t cap,
                                                             const unsigned long long* __restrict__ words, ExSum* __restrict__ tiles) {
    __shared__ ExSum s_wave[kExThreads / 64];
    unsigned long long len[kExRecsPerLane];
    const uint32_t n_runs = sp_live_runs(words, cap);
    const ExSum s{sp_lens(vals, pre, n_runs, words[kExNl], ((uint64_t)blockIdx.x * kExThreads + threadIdx.x) * kExRecsPerLane, len), 0u, 0u};
    const ExSum all = block_sum<kExThreads / 64>(s, s_wave);
    if (threadIdx.x == 0) tiles[blockIdx.x] = all;
}

// sorted run j: source bytes from run_src[j] on -> output bytes [run_dst[j], run_dst[j + 1]); run_dst[n_runs] = the output's bytes
__global__ __launch_bounds__(kExThreads) void k_sp_dst_write(const uint32_t* __restrict__ vals, const uint64_t* __restrict__ pre, const uint64_t* __restrict__ src,
                                                             uint32_t cap, uint64_t n_tiles, const ExSum* __restrict__ base, uint64_t* __restrict__ run_src,
                                                             uint64_t* __restrict__ run_dst, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long s_wave[kExThreads / 64];
    unsigned long long len[kExRecsPerLane];
    const uint32_t n_runs = sp_live_runs(words, cap);
    const unsigned long long nl = words[kExNl];
    const uint64_t j0 = ((uint64_t)blockIdx.x * kExThreads + threadIdx.x) * kExRecsPerLane;
    const unsigned long long sum = sp_lens(vals, pre, n_runs, nl, j0, len);
    unsigned long long at = block_prefix_excl<kExThreads / 64>(sum, threadIdx.x & 63u, threadIdx.x >> 6, s_wave);
    if (blockIdx.x < n_tiles) {
        at += base[blockIdx.x].a;
#pragma unroll
        for (uint32_t u = 0; u < kExRecsPerLane; ++u) {
            if (j0 + u >= n_runs) break;
            const uint32_t v = vals[j0 + u];
            run_dst[j0 + u] = at;
            run_src[j0 + u] = v < n_runs ? src[v] : 0ull;
            at += len[u];
            if (nl && v + 1u == n_runs) words[kSpNlAt] = at - 1ull;   // (one lane of the grid: the last run in record order)
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) run_dst[n_runs] = n_runs ? words[kSpOut] : 0ull;
}

// bin_off[b], b = 0 .. n_bins: where the first sorted run of a bin >= b begins in the output
__global__ __launch_bounds__(kExThreads) void k_sp_bin_off(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ run_dst, uint32_t cap, uint32_t n_bins,
                                                           const unsigned long long* __restrict__ words, uint64_t* __restrict__ bin_off) {
    const uint64_t b = (uint64_t)blockIdx.x * kExThreads + threadIdx.x;
    if (b > n_bins) return;
    const uint32_t n_runs = sp_live_runs(words, cap);
    uint32_t lo = 0, hi = n_runs;                          // the first j of [0, n_runs] with keys[j] >= b
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < b) lo = mid + 1u; else hi = mid; }
    bin_off[b] = run_dst[lo];
}

__global__ __launch_bounds__(kExThreads) void k_sp_copy(const uint8_t* __restrict__ text, uint64_t n_text, const uint64_t* __restrict__ run_src,
                                                        const uint64_t* __restrict__ run_dst, uint32_t cap, const unsigned long long* __restrict__ words,
                                                        uint8_t* __restrict__ out) {
    __shared__ uint32_t s_range[2];
    const uint32_t n_runs = sp_live_runs(words, cap);
    const uint64_t n_out = n_runs ? words[kSpOut] : 0ull, nl_at = words[kSpNlAt];
    const uint64_t o_wg = (uint64_t)blockIdx.x * kExStretch;
    if (o_wg >= n_out) return;                             // (uniform.  The grid is sized by the text: the output may be far shorter)
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
        if (o + 16ull <= re && nl_at - o >= 16ull) {       // (nl_at < o wraps to a large number; ~0 is no newline)
            // inside one run and clear of the appended newline: the 16 source bytes, out of the two aligned groups that hold them
            v = ex_gather16(text, n_text, rs + (o - rd));
        } else {
            // across runs, the appended newline or the output's end: byte by byte (zeros behind the end: the buffer is whole stretches)
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t b = 0; b < 16u; ++b) {
                const uint64_t pos = o + b;
                uint32_t byte = 0u;
                if (pos < n_out) {
                    while (pos >= re && i + 1u < n_runs) { ++i; rs = run_src[i]; rd = re; re = run_dst[i + 1]; }   // (runs are not empty and run_dst[n_runs] = n_out)
                    const uint64_t from = rs + (pos - rd);
                    byte = pos == nl_at ? (uint32_t)'\n' : (from < n_text ? text[from] : 0u);
                }
                w[b >> 2] |= byte << (8 * (b & 3u));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(out + o) = v;
    }
}

int sp_mark(spsp_ctx* ctx, int i) {
    if (!ctx->timing) return SPSP_OK;
    if (!ctx->sp_ev[i]) SPSP_HIP(hipEventCreate(&ctx->sp_ev[i]));
    SPSP_HIP(hipEventRecord(ctx->sp_ev[i], ctx->stream));
    ctx->sp_marked |= 1u << i;
    return SPSP_OK;
}

// the digits the sort needs for keys below n_bins, as bits
uint32_t sp_sort_bits(uint32_t n_bins) {
    uint32_t bits = 0;
    while (bits < 32u && ((uint64_t)(n_bins - 1u) >> bits) != 0ull) bits += 8u;
    return bits;
}

}  // namespace

int records_split_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_begin, uint32_t n_rec, const uint32_t* h_bin, uint32_t n_bins,
                       uint8_t** d_out, uint64_t* n_out, uint64_t* h_bin_off, uint64_t* h_bin_records, bool* fastq) {
    int rc;
    *d_out = nullptr; *n_out = 0;
    if (n_bins == 0 || n_bins > kSpMaxBins) { set_error("split: n_bins must be 1 .. %u (n_bins = %u)", kSpMaxBins, n_bins); return SPSP_ERR_ARG; }
    std::fill(h_bin_off, h_bin_off + (size_t)n_bins + 1, 0ull);
    std::fill(h_bin_records, h_bin_records + n_bins, 0ull);
    if (n_rec > 0xfffffff0u) { set_error("too many records for one call (%u)", n_rec); return SPSP_ERR_OVERFLOW; }
    const bool own = d_begin == nullptr;
    // the bins, on the host: the refusal, bin_records, and the most runs the device can find.  With starts of its own no record
    // is empty (but the empty text's one), so a run begins only where the bin changes; a caller's ranges may be empty anywhere
    uint64_t cap64 = 0;
    uint32_t prev = kSpDrop;
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint32_t b = h_bin[r];
        if (b != kSpDrop) {
            if (b >= n_bins) {
                std::fill(h_bin_records, h_bin_records + n_bins, 0ull);
                set_error("split: bin[%u] = %u, n_bins = %u", r, b, n_bins);
                return SPSP_ERR_ARG;
            }
            ++h_bin_records[b];
            if (!own || b != prev) ++cap64;
        }
        prev = b;
    }
    const uint32_t cap = (uint32_t)cap64;
    uint64_t n_tiles = 0;
    if ((rc = ex_front(ctx, d_text, n_text, &n_tiles))) return rc;
    const uint64_t n_rtiles = ((uint64_t)n_rec + kExRecTile - 1) / kExRecTile, n_stiles = ((uint64_t)cap + kExRecTile - 1) / kExRecTile;
    const uint64_t grid = (n_text + 1 + kExStretch - 1) / kExStretch;   // the output is the text and one newline at the most
    if (grid > 0x7fffffffull) { set_error("text too large for one call"); return SPSP_ERR_OVERFLOW; }
    // the run table: pre (cap + 1) | src | keys twice | run_src | run_dst (cap + 1) | vals twice
    const size_t c1 = (size_t)cap + 1, sums = (size_t)std::max(std::max(n_tiles, n_rtiles), n_stiles) + 1;
    if ((rc = ctx->ex_tiles.reserve(sums * sizeof(ExSum))) || (rc = ctx->ex_bases.reserve(sums * sizeof(ExSum))) || (rc = ctx->sp_bin.reserve((size_t)n_rec * 4 + 64)) ||
        (rc = ctx->sp_runs.reserve(c1 * (6 * 8 + 2 * 4))) || (rc = ctx->sp_off.reserve(((size_t)n_bins + 1) * 8)) ||
        (rc = ctx->ex_out.reserve((size_t)grid * kExStretch)) || (rc = sp_mark(ctx, 0))) return rc;
    if (own) {
        if ((rc = ex_count_launch(ctx, d_text, n_text, n_tiles)) || (rc = ex_starts_launch(ctx, d_text, n_text, n_tiles, n_rec))) return rc;
        d_begin = ctx->ex_begin.as<uint64_t>();
    } else {
        if ((rc = ctx->ex_words.reserve(kExWords * 8))) return rc;
        SPSP_HIP(hipMemsetAsync(ctx->ex_words.p, 0, kExWords * 8, ctx->stream));
    }
    if ((rc = sp_mark(ctx, 1))) return rc;
    unsigned long long* words = ctx->ex_words.as<unsigned long long>();
    uint32_t* bin = ctx->sp_bin.as<uint32_t>();
    uint64_t* pre = ctx->sp_runs.as<uint64_t>();
    uint64_t *src = pre + c1, *keys = src + c1, *keys_tmp = keys + c1, *run_src = keys_tmp + c1, *run_dst = run_src + c1;
    uint32_t *vals = reinterpret_cast<uint32_t*>(run_dst + c1), *vals_tmp = vals + c1;
    uint64_t* bin_off = ctx->sp_off.as<uint64_t>();
    ExSum *tiles = ctx->ex_tiles.as<ExSum>(), *bases = ctx->ex_bases.as<ExSum>();
    if (n_rec) SPSP_HIP(hipMemcpyAsync(bin, h_bin, (size_t)n_rec * 4, hipMemcpyHostToDevice, ctx->stream));
    SPSP_HIP(hipMemsetAsync(keys, 0xFF, c1 * 8, ctx->stream));   // (the places behind the runs the device finds: all ones, behind every run once sorted)
    if (n_rtiles) hipLaunchKernelGGL(k_sp_rec_tiles, dim3((uint32_t)n_rtiles), dim3(kExThreads), 0, ctx->stream, d_begin, (const uint32_t*)bin, n_rec, n_text, tiles, words);
    if ((rc = ex_scan_launch(ctx, tiles, n_rtiles, bases, words + kExSrc))) return rc;
    hipLaunchKernelGGL(k_sp_rec_write, dim3((uint32_t)std::max<uint64_t>(n_rtiles, 1)), dim3(kExThreads), 0, ctx->stream, d_text, n_text, d_begin, (const uint32_t*)bin,
                       n_rec, n_rtiles, (const ExSum*)bases, cap, src, pre, keys, vals, words);
    SPSP_HIP(hipGetLastError());
    if ((rc = sp_mark(ctx, 2)) || (rc = radix_sort_pairs(ctx, &keys, &vals, keys_tmp, vals_tmp, cap, sp_sort_bits(n_bins))) || (rc = sp_mark(ctx, 3))) return rc;
    if (n_stiles) hipLaunchKernelGGL(k_sp_len_tiles, dim3((uint32_t)n_stiles), dim3(kExThreads), 0, ctx->stream, (const uint32_t*)vals, (const uint64_t*)pre, cap,
                                     (const unsigned long long*)words, tiles);
    if ((rc = ex_scan_launch(ctx, tiles, n_stiles, bases, words + kSpOut))) return rc;
    hipLaunchKernelGGL(k_sp_dst_write, dim3((uint32_t)std::max<uint64_t>(n_stiles, 1)), dim3(kExThreads), 0, ctx->stream, (const uint32_t*)vals, (const uint64_t*)pre,
                       (const uint64_t*)src, cap, n_stiles, (const ExSum*)bases, run_src, run_dst, words);
    hipLaunchKernelGGL(k_sp_bin_off, dim3(n_bins / kExThreads + 1), dim3(kExThreads), 0, ctx->stream, (const uint64_t*)keys, (const uint64_t*)run_dst, cap, n_bins,
                       (const unsigned long long*)words, bin_off);
    SPSP_HIP(hipGetLastError());
    if ((rc = sp_mark(ctx, 4))) return rc;
    hipLaunchKernelGGL(k_sp_copy, dim3((uint32_t)grid), dim3(kExThreads), 0, ctx->stream, d_text, n_text, (const uint64_t*)run_src, (const uint64_t*)run_dst, cap,
                       (const unsigned long long*)words, ctx->ex_out.as<uint8_t>());
    SPSP_HIP(hipGetLastError());
    if ((rc = sp_mark(ctx, 5))) return rc;
    uint64_t h[kExWords];
    SPSP_HIP(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(h_bin_off, bin_off, ((size_t)n_bins + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    const hipError_t waited = hipStreamSynchronize(ctx->stream);   // the wait that brings back the call's words and bin_off
    if (waited != hipSuccess) std::fill(h_bin_off, h_bin_off + (size_t)n_bins + 1, 0ull);
    SPSP_HIP(waited);
    if (ctx->timing && (ctx->sp_marked & 63u) == 63u)
        for (int i = 0; i < 5; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ctx->sp_ev[i], ctx->sp_ev[i + 1])); ctx->sp_ms[i] += ms; }
    ctx->sp_marked = 0;
    const auto refuse = [&](int code) {
        std::fill(h_bin_off, h_bin_off + (size_t)n_bins + 1, 0ull);
        std::fill(h_bin_records, h_bin_records + n_bins, 0ull);
        return code;
    };
    if (own) {
        if (h[kExBad] & 1ull) return refuse(ex_refuse_lines(h[kExUnits] + 1));
        if (h[kExRecs] != n_rec) {
            set_error("split: the text holds %llu record(s), the bins are for %u", (unsigned long long)h[kExRecs], n_rec);
            return refuse(SPSP_ERR_ARG);
        }
    }
    if (h[kExBad] & 2ull) { set_error("split: d_begin must not decrease and must end inside the text"); return refuse(SPSP_ERR_ARG); }
    if (h[kExBad]) { set_error("split: the device found more runs than the bins allow (%llu, %u)", (unsigned long long)(uint32_t)h[kExRunsKept], cap); return refuse(SPSP_ERR_ARG); }
    *d_out = ctx->ex_out.as<uint8_t>();
    *n_out = h_bin_off[n_bins];
    if (fastq) *fastq = own ? h[kExFastq] != 0 : false;
    return SPSP_OK;
}

int ExtractRun::split_text(spsp_ctx* side, const uint8_t* d_text, uint64_t n_text, uint32_t n_records, const uint32_t* bin, uint32_t bins) {
    int rc;
    n_bins = bins;
    if (n_bins == 0 || n_bins > kSpMaxBins) { set_error("split: n_bins must be 1 .. %u (n_bins = %u)", kSpMaxBins, n_bins); return SPSP_ERR_ARG; }
    bin_off.assign((size_t)n_bins + 1, 0);
    bin_records.assign(n_bins, 0);
    uint8_t* d_out = nullptr;
    uint64_t n_out = 0;
    // (the ingest has told the road n_records: the starts are made for as many, with no wait of their own)
    if ((rc = records_split_impl(side, d_text, n_text, nullptr, n_records, bin, n_bins, &d_out, &n_out, bin_off.data(), bin_records.data(), &fastq))) return rc;
    n_rec = n_kept = n_records;
    out.resize((size_t)n_out);
    if (n_out) SPSP_HIP(hipMemcpyAsync(out.data(), d_out, (size_t)n_out, hipMemcpyDeviceToHost, side->stream));   // every kept byte comes back once
    SPSP_HIP(hipStreamSynchronize(side->stream));
    return SPSP_OK;
}

int split_write(spsp_ctx* ctx, ExtractRun* run, ExtractRun* mates, const char* const* bin_names, const char* last_name, const char* out_prefix, int chatter) {
    const double t = now_s();
    ExtractRun* side[2] = {run, mates};
    std::string suffix[2];
    for (int s = 0; s < 2; ++s)
        if (side[s]) suffix[s] = std::string(side[s]->fastq ? ".fq" : ".fa") + (side[s]->gz ? ".gz" : "");
    std::vector<std::string> written;
    int rc = SPSP_OK;
    run->bins_written = 0;
    for (uint32_t b = 0; b < run->n_bins && !rc; ++b) {
        if (!run->bin_records[b]) continue;
        ++run->bins_written;
        for (int s = 0; s < 2 && !rc; ++s) {
            if (!side[s]) continue;
            const std::string path = split_file_name(out_prefix, b, run->n_bins, last_name, side[s]->tag, suffix[s].c_str());
            written.push_back(path);
            rc = write_bytes(path.c_str(), side[s]->out.data() + side[s]->bin_off[b], side[s]->bin_off[b + 1] - side[s]->bin_off[b], side[s]->gz);
        }
    }
    ctx->stages.csv_gzip_s += now_s() - t;
    char* text = nullptr; uint64_t len = 0;
    if (!rc) {
        const char* slash = strrchr(out_prefix, '/');      // (the manifest names the files as they lie beside it)
        rc = spsp_split_csv_host(slash ? slash + 1 : out_prefix, bin_names, last_name, run->n_bins, run->bin_records.data(), run->bin_off.data(),
                                 suffix[0].c_str(), mates ? mates->bin_off.data() : nullptr, suffix[1].c_str(), &text, &len);
    }
    if (!rc) rc = write_csv_gz(ctx, text, len, out_prefix, "_split.csv.gz", now_s());
    if (rc) { for (const std::string& path : written) (void)remove(path.c_str()); return rc; }   // (nothing is left of a split that failed)
    if (chatter) {
        if (mates) printf("split %s: %llu bin(s) written, %llu pair(s), %llu + %llu byte(s)\n", run->what, (unsigned long long)run->bins_written,
                          (unsigned long long)run->n_rec, (unsigned long long)run->out.size(), (unsigned long long)mates->out.size());
        else printf("split %s: %llu bin(s) written, %llu record(s), %llu byte(s)\n", run->what, (unsigned long long)run->bins_written, (unsigned long long)run->n_rec,
                    (unsigned long long)run->out.size());
        fflush(stdout);
    }
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_records_split_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, const void* d_begin, uint32_t n_rec, const uint32_t* h_bin,
                                         uint32_t n_bins, void** d_out, uint64_t* n_out, uint64_t* h_bin_off, uint64_t* h_bin_records) {
    if (!ctx || !d_out || !n_out || !h_bin_off || !h_bin_records || (n_text && !d_text) || (n_rec && !h_bin)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint8_t* o = nullptr;
    const int rc = records_split_impl(ctx, (const uint8_t*)d_text, n_text, (const uint64_t*)d_begin, n_rec, h_bin, n_bins, &o, n_out, h_bin_off, h_bin_records, nullptr);
    ctx->sp_marked = 0;
    *d_out = o;
    return rc;
}

extern "C" int spsp_split_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (int i = 0; i < 5; ++i) { ms[i] = ctx->sp_ms[i]; ctx->sp_ms[i] = 0; }
    return SPSP_OK;
}
