// Segments as sequence on the GPU: the chosen segments of a windowed run written as FASTA from the cleaned bases the side context
// still holds (not in the reference, which has no record passes).  The rule is in include/spsp.h ("segments as sequence"); this
// file is its device form, and the tail of a windowed driver that uses it.
//
// The host makes the headers (only it holds the names) and prefix-sums header and body lengths into seg_out[n_seg + 1]; one upload
// carries seg_out, the segments' source starts, the headers' offsets and the headers.  k_sg_write, the one launch, is balanced by
// OUTPUT bytes on the extraction's schedule: a workgroup owns a stretch of 16 KiB of the text, finds the segments that cross it
// with two binary searches over seg_out, copies their slice of the three tables into LDS (up to kSgLdsSegs segments; a stretch of
// more, which takes segments of a few bases each, reads the tables from memory), and every lane writes 16-byte-aligned 16-byte
// stores, each found by a search over the slice in LDS -- no chain of dependent loads from memory per store.
// Inside a body, output byte t is '\n' when t % 81 == 80 or t is the body's last byte, else base t - t / 81 of the segment.  A
// store that lies wholly inside one body and holds at most one newline takes the 16 (or 15) bases from t0 - t0 / 81 on: ASCII by
// ex_gather16 (two aligned loads and a byte shift), packed by one funnel shift of two source dwords and four byte permutes over
// 'A','C','T','G'; the newline goes in by a one-byte funnel of the dwords behind it and one byte permute in the dword that holds
// it.  A store that holds header bytes, spans segments, holds a line's newline AND the body's last, or ends the text is assembled
// byte by byte.  Loads are guarded by n_bases; the output buffer is whole stretches, as many as the grid has workgroups: no store
// can leave it.  Ordering is by the stream; no atomics; plain vector stores.
#include <algorithm>
#include <string>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

static_assert(kSgStores * kSgThreads * 16 == kSgStretch && kSgLine == SPSP_SEGMENTS_LINE && kSgLine + 1 > 16, "a stretch is whole 16-byte stores; a store holds one line end at the most");
constexpr uint32_t kSgRow = kSgLine + 1;                   // bytes of a full line
constexpr uint32_t kSgLetters = 'A' | ('C' << 8) | ('T' << 16) | ((uint32_t)'G' << 24);   // the letter of code c is byte c

__device__ __forceinline__ uint64_t sg_rows(uint64_t t) { return t <= 0xffffffffull ? (uint64_t)((uint32_t)t / kSgRow) : t / kSgRow; }

// base g of the text as a letter (g < n_bases is the caller's)
template <bool PACKED>
__device__ __forceinline__ uint32_t sg_base(const uint8_t* __restrict__ bases, uint64_t g) {
    if (!PACKED) return bases[g];
    const uint32_t code = (reinterpret_cast<const uint32_t*>(bases)[g >> 4] >> (30u - 2u * (uint32_t)(g & 15ull))) & 3u;
    return (kSgLetters >> (8u * code)) & 0xffu;
}

// the 16 letters from base s on (those behind n_bases are not letters: the caller drops them)
template <bool PACKED>
__device__ __forceinline__ void sg_letters16(const uint8_t* __restrict__ bases, uint64_t n_bases, uint64_t s, uint32_t (&w)[4]) {
    if (!PACKED) {
        const uint4 v = ex_gather16(bases, n_bases, s);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(bases);
    const uint64_t n_words = (n_bases + 15ull) >> 4, q = s >> 4;
    const uint32_t sh = 2u * (uint32_t)(s & 15ull);
    const uint32_t hi = q < n_words ? src[q] : 0u;
    const uint32_t lo = sh && q + 1 < n_words ? src[q + 1] : 0u;
    const uint32_t x = sh ? (hi << sh) | (lo >> (32u - sh)) : hi;   // (one v_alignbit_b32): 16 codes, the first in bits 31:30
#pragma unroll
    for (uint32_t g = 0; g < 4u; ++g) {
        const uint32_t c = (x >> (24u - 8u * g)) & 0xffu;  // four codes, the first in bits 7:6: one selector byte each
        const uint32_t sel = (c >> 6) | (((c >> 4) & 3u) << 8) | (((c >> 2) & 3u) << 16) | ((c & 3u) << 24);
        w[g] = __builtin_amdgcn_perm(0u, kSgLetters, sel);
    }
}

// '\n' put in at byte nl < 16: the bytes in front stay, the bytes behind move up by one (the 16th drops out)
__device__ __forceinline__ void sg_newline(uint32_t (&w)[4], uint32_t nl) {
    const uint32_t up[4] = {w[0] << 8, __builtin_amdgcn_alignbit(w[1], w[0], 24u), __builtin_amdgcn_alignbit(w[2], w[1], 24u), __builtin_amdgcn_alignbit(w[3], w[2], 24u)};
    const uint32_t dn = nl >> 2, e = 8u * (nl & 3u), low = (1u << e) - 1u;
    const uint32_t sel = (0x07060504u & ~low) | (0x03020100u & low);   // bytes in front of the newline from w, the others from up
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {
        if (d > dn) w[d] = up[d];
        else if (d == dn) w[d] = (__builtin_amdgcn_perm(up[d], w[d], sel) & ~(0xffu << e)) | ((uint32_t)'\n' << e);
    }
}

// the stores of one stretch.  t_out[0 .. n_loc], t_src[0 .. n_loc), t_hdr[0 .. n_loc]: the slice of the tables of the n_loc segments
// that cross it (in LDS or in memory); t_out[0] <= o_wg, and the stretch's last byte of text lies in front of t_out[n_loc]
template <bool PACKED>
__device__ __forceinline__ void sg_stores(const uint8_t* __restrict__ bases, uint64_t n_bases, const uint64_t* t_out, const uint64_t* t_src, const uint64_t* t_hdr,
                                          uint32_t n_loc, const uint8_t* __restrict__ headers, uint64_t n_out, uint64_t o_wg, uint8_t* __restrict__ out) {
#pragma unroll
    for (uint32_t it = 0; it < kSgStores; ++it) {
        const uint64_t o = o_wg + (uint64_t)(it * kSgThreads + threadIdx.x) * 16ull;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (o < n_out && n_loc != 0u) {
            uint32_t i = ex_find(t_out, 0u, n_loc, o);
            uint64_t so = t_out[i], se = t_out[i + 1], h0 = t_hdr[i], bs = so + (t_hdr[i + 1] - h0);
            bool fast = false;
            if (o >= bs && o + 16ull <= se) {
                const uint64_t t0 = o - bs, rows = sg_rows(t0);
                const uint32_t p = kSgLine - (uint32_t)(t0 - rows * kSgRow);   // the store's byte p is a line's newline where p < 16
                const bool last = o + 16ull == se;                // byte 15 is the body's last: a newline as well
                if (!(last && p < 15u)) {
                    fast = true;
                    sg_letters16<PACKED>(bases, n_bases, t_src[i] + (t0 - rows), w);
                    const uint32_t nl = p < 16u ? p : (last ? 15u : 16u);
                    if (nl < 16u) sg_newline(w, nl);
                }
            }
            if (!fast) {
                // header bytes, several segments, two newlines or the text's end: byte by byte (zeros behind the end)
#pragma unroll
                for (uint32_t b = 0; b < 16u; ++b) {
                    const uint64_t pos = o + b;
                    if (pos >= n_out) continue;
                    while (pos >= se) { ++i; so = se; se = t_out[i + 1]; h0 = t_hdr[i]; bs = so + (t_hdr[i + 1] - h0); }   // (i stays below n_loc)
                    uint32_t byte;
                    if (pos < bs) byte = headers[h0 + (pos - so)];
                    else {
                        const uint64_t t = pos - bs, rows = sg_rows(t), g = t_src[i] + (t - rows);
                        const bool nl = t + 1 == se - bs || t - rows * kSgRow == kSgLine;
                        byte = nl ? (uint32_t)'\n' : (g < n_bases ? sg_base<PACKED>(bases, g) : 0u);
                    }
                    w[b >> 2] |= byte << (8u * (b & 3u));
                }
            }
        }
        *reinterpret_cast<uint4*>(out + o) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <bool PACKED>
__global__ __launch_bounds__(kSgThreads) void k_sg_write(const uint8_t* __restrict__ bases, uint64_t n_bases, const uint64_t* __restrict__ seg_out,
                                                         const uint64_t* __restrict__ seg_src, const uint64_t* __restrict__ hdr_off,
                                                         const uint8_t* __restrict__ headers, uint32_t n_seg, uint64_t n_out, uint8_t* __restrict__ out) {
    __shared__ uint32_t s_range[2];
    __shared__ uint64_t s_out[kSgLdsSegs + 1], s_src[kSgLdsSegs + 1], s_hdr[kSgLdsSegs + 1];
    const uint64_t o_wg = (uint64_t)blockIdx.x * kSgStretch;
    const bool any = o_wg < n_out && n_seg != 0u;          // (uniform.  The one stretch of an empty text is zeros)
    if (any) {
        if (threadIdx.x == 0u) s_range[0] = ex_find(seg_out, 0u, n_seg, o_wg);
        if (threadIdx.x == 64u) s_range[1] = ex_find(seg_out, 0u, n_seg, (o_wg + kSgStretch < n_out ? o_wg + kSgStretch : n_out) - 1ull);
    }
    __syncthreads();
    const uint32_t i_lo = any ? s_range[0] : 0u, n_loc = any ? s_range[1] + 1u - i_lo : 0u;
    const bool staged = n_loc <= kSgLdsSegs;               // (uniform)
    if (staged)
        for (uint32_t j = threadIdx.x; j <= n_loc && n_loc != 0u; j += kSgThreads) {
            s_out[j] = seg_out[i_lo + j]; s_hdr[j] = hdr_off[i_lo + j];
            s_src[j] = j < n_loc ? seg_src[i_lo + j] : 0ull;
        }
    __syncthreads();
    if (staged) sg_stores<PACKED>(bases, n_bases, s_out, s_src, s_hdr, n_loc, headers, n_out, o_wg, out);
    else sg_stores<PACKED>(bases, n_bases, seg_out + i_lo, seg_src + i_lo, hdr_off + i_lo, n_loc, headers, n_out, o_wg, out);
}

}  // namespace

static int sg_collect_ms(spsp_ctx* ctx) {
    if (!ctx->sg_marked) return SPSP_OK;
    SPSP_HIP(hipEventSynchronize(ctx->sg_ev[1]));
    float ms = 0;
    SPSP_HIP(hipEventElapsedTime(&ms, ctx->sg_ev[0], ctx->sg_ev[1]));
    ctx->sg_ms += ms; ctx->sg_marked = false;
    return SPSP_OK;
}

int segments_write_impl(spsp_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, bool packed, const uint64_t* h_src, const uint64_t* h_len, const uint8_t* h_headers,
                        const uint64_t* h_hdr_off, uint64_t n_seg, uint8_t** d_out, uint64_t* n_out) {
    int rc;
    *d_out = nullptr; *n_out = 0;
    if (n_seg > 0xfffffff0ull) { set_error("segments: too many segments for one call (%llu)", (unsigned long long)n_seg); return SPSP_ERR_OVERFLOW; }
    if (((uintptr_t)d_bases & 15u) != 0) { set_error("d_bases must be 16-byte aligned"); return SPSP_ERR_ARG; }
    // everything is held before anything is launched: no segment leaves the bases, no header lies in front of the one before
    const uint64_t n_blob = h_hdr_off[n_seg] - h_hdr_off[0];
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_seg; ++i) {
        if (h_len[i] == 0 || h_len[i] > n_bases || h_src[i] > n_bases - h_len[i]) {
            set_error("segments: segment %llu (%llu base(s) from %llu on) has no bases or leaves the %llu bases", (unsigned long long)i, (unsigned long long)h_len[i],
                      (unsigned long long)h_src[i], (unsigned long long)n_bases);
            return SPSP_ERR_ARG;
        }
        if (h_hdr_off[i] > h_hdr_off[i + 1]) { set_error("segments: the headers' offsets must not decrease (segment %llu)", (unsigned long long)i); return SPSP_ERR_ARG; }
        total += (h_hdr_off[i + 1] - h_hdr_off[i]) + h_len[i] + (h_len[i] + kSgLine - 1) / kSgLine;
    }
    const uint64_t grid = std::max<uint64_t>((total + kSgStretch - 1) / kSgStretch, 1);
    if (grid > 0x7fffffffull) { set_error("segments: %llu bytes of text are too many for one call", (unsigned long long)total); return SPSP_ERR_OVERFLOW; }
    const size_t rows = (size_t)n_seg + 1, tab_bytes = rows * 24 + (size_t)n_blob;
    if ((rc = ctx->sg_tab.reserve(tab_bytes + 16)) || (rc = ctx->sg_out.reserve((size_t)grid * kSgStretch))) return rc;
    // the one upload: seg_out, the source starts, the headers' offsets (from 0), the headers.  The host copy stays with the context
    ctx->sg_host.resize(tab_bytes);
    uint64_t *t_out = reinterpret_cast<uint64_t*>(ctx->sg_host.data()), *t_src = t_out + rows, *t_hdr = t_src + rows;
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_seg; ++i) {
        t_out[i] = at; t_src[i] = h_src[i]; t_hdr[i] = h_hdr_off[i] - h_hdr_off[0];
        at += (h_hdr_off[i + 1] - h_hdr_off[i]) + h_len[i] + (h_len[i] + kSgLine - 1) / kSgLine;
    }
    t_out[n_seg] = at; t_src[n_seg] = 0; t_hdr[n_seg] = n_blob;
    if (n_blob) memcpy(ctx->sg_host.data() + rows * 24, h_headers + h_hdr_off[0], (size_t)n_blob);
    SPSP_HIP(hipMemcpyAsync(ctx->sg_tab.p, ctx->sg_host.data(), tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t* d_tab = ctx->sg_tab.as<uint64_t>();
    const uint8_t* d_hdr = ctx->sg_tab.as<uint8_t>() + rows * 24;
    if (ctx->timing) {
        if ((rc = sg_collect_ms(ctx))) return rc;          // (only then: an earlier call's span is read before its events are used again)
        for (hipEvent_t& e : ctx->sg_ev) if (!e) SPSP_HIP(hipEventCreate(&e));
        SPSP_HIP(hipEventRecord(ctx->sg_ev[0], ctx->stream));
    }
    if (packed) hipLaunchKernelGGL(k_sg_write<true>, dim3((uint32_t)grid), dim3(kSgThreads), 0, ctx->stream, d_bases, n_bases, d_tab, d_tab + rows, d_tab + 2 * rows, d_hdr,
                                   (uint32_t)n_seg, total, ctx->sg_out.as<uint8_t>());
    else hipLaunchKernelGGL(k_sg_write<false>, dim3((uint32_t)grid), dim3(kSgThreads), 0, ctx->stream, d_bases, n_bases, d_tab, d_tab + rows, d_tab + 2 * rows, d_hdr,
                            (uint32_t)n_seg, total, ctx->sg_out.as<uint8_t>());
    SPSP_HIP(hipGetLastError());
    if (ctx->timing) { SPSP_HIP(hipEventRecord(ctx->sg_ev[1], ctx->stream)); ctx->sg_marked = true; }
    *d_out = ctx->sg_out.as<uint8_t>(); *n_out = total;
    return SPSP_OK;
}

int windows_tail(spsp_ctx* side, WindowsRun* run, const RecordsAsk& ask, uint32_t k, std::vector<uint32_t>& call, const std::vector<uint32_t>& keys,
                 const std::vector<uint32_t>& hit_keys, std::vector<uint32_t>& support, uint32_t n_bins, const std::vector<std::string>& names,
                 const char* const* call_names, const char* last_name) {
    int rc;
    const uint32_t n_rec = (uint32_t)(run->rec_off.size() - 1);
    run->k = k; run->n_bins = n_bins; run->want_fasta = ask.segments_what != nullptr;
    if ((rc = segments_ask_check(ask, 0, n_bins))) return rc;   // (<b> of a taxonomy: the nodes are counted by now)
    if (ask.smooth && (rc = spsp_windows_smooth_host(call.data(), support.data(), run->first_win.data(), n_rec, n_bins, ask.smooth, &run->n_changed))) return rc;
    spsp_segment_row* segs = nullptr; uint64_t n_segs = 0;
    run->mosaic.assign(n_rec, spsp_mosaic_row{});
    spsp_mosaic_row none_row{};
    if ((rc = spsp_windows_segments_host(call.data(), keys.data(), hit_keys.data(), support.data(), run->first_win.data(), run->rec_off.data(), n_rec, k, run->window,
                                         n_bins, &segs, &n_segs, n_rec ? run->mosaic.data() : &none_row))) return rc;
    run->segments.assign(segs, segs + n_segs);
    spsp_free(segs);
    std::vector<const char*> name_ptr(names.size());
    for (size_t r = 0; r < names.size(); ++r) name_ptr[r] = names[r].c_str();
    char *seg_text = nullptr, *mos_text = nullptr; uint64_t seg_len = 0, mos_len = 0;
    if ((rc = spsp_segments_csv_host(run->segments.data(), n_segs, name_ptr.data(), n_rec, call_names, last_name, n_bins, &seg_text, &seg_len))) return rc;
    run->seg_csv.assign(seg_text, (size_t)seg_len);
    free(seg_text);
    if ((rc = spsp_mosaic_csv_host(run->mosaic.data(), n_rec, name_ptr.data(), call_names, last_name, n_bins, ask.precision, &mos_text, &mos_len))) return rc;
    run->mos_csv.assign(mos_text, (size_t)mos_len);
    free(mos_text);
    run->want_bed = ask.raw != 0;
    if (ask.raw) {
        // the two ends of every segment that has bases, as global kept-base indices: ascending as they come, the segments being in
        // record order and within a record in position order.  ONE lift over the raw text the side context still holds
        std::vector<uint64_t> at;
        at.reserve((size_t)n_segs * 2 + 1);
        for (const spsp_segment_row& g : run->segments)
            if (g.end > g.begin) { at.push_back(run->rec_off[g.record] + g.begin); at.push_back(run->rec_off[g.record] + g.end - 1); }
        std::vector<uint64_t> lifted(at.size() + 1, 0);
        uint32_t text_rec = 0;
        if ((rc = records_lift_impl(side, run->d_text, run->n_text, run->n_bases, at.data(), at.size(), lifted.data(), nullptr, nullptr, &text_rec))) return rc;
        run->raw_begin.assign((size_t)n_segs, 0); run->raw_end.assign((size_t)n_segs, 0);
        run->n_lifted = 0; run->raw_excess = 0;
        size_t j = 0;
        for (uint64_t i = 0; i < n_segs; ++i) {
            const spsp_segment_row& g = run->segments[i];
            if (g.end == g.begin) continue;
            run->raw_begin[i] = lifted[j]; run->raw_end[i] = lifted[j + 1] + 1; j += 2;
            ++run->n_lifted;
            run->raw_excess += (run->raw_end[i] - run->raw_begin[i]) - (g.end - g.begin);
        }
        char* bed_text = nullptr; uint64_t bed_len = 0;
        if ((rc = spsp_segments_bed_host(run->segments.data(), n_segs, run->raw_begin.data(), run->raw_end.data(), name_ptr.data(), n_rec, call_names, last_name, n_bins,
                                         &bed_text, &bed_len))) return rc;
        run->bed.assign(bed_text, (size_t)bed_len);
        free(bed_text);
    }
    if (!ask.segments_what) return SPSP_OK;
    std::vector<uint8_t> keep(n_segs ? (size_t)n_segs : 1, 0);
    if ((rc = spsp_segments_select_host(run->segments.data(), n_segs, n_rec ? run->mosaic.data() : &none_row, n_rec, n_bins, ask.segments_what, ask.segments_min,
                                        keep.data(), &run->n_written, &run->bases_written))) return rc;
    std::vector<uint64_t> src, len, hdr_off(1, 0);
    std::string headers;
    for (uint64_t i = 0; i < n_segs; ++i) {
        if (!keep[i]) continue;
        const spsp_segment_row& g = run->segments[i];
        src.push_back(run->rec_off[g.record] + g.begin);
        len.push_back(g.end - g.begin);
        segment_header(g, name_ptr[g.record], call_names, last_name, n_bins, &headers);
        hdr_off.push_back(headers.size());
    }
    uint8_t* d_out = nullptr; uint64_t n_out = 0;
    if ((rc = segments_write_impl(side, run->d_bases, run->n_bases, run->packed, src.data(), len.data(), reinterpret_cast<const uint8_t*>(headers.data()), hdr_off.data(),
                                  src.size(), &d_out, &n_out))) return rc;
    run->fasta.resize((size_t)n_out);
    if (n_out) SPSP_HIP(hipMemcpyAsync(run->fasta.data(), d_out, (size_t)n_out, hipMemcpyDeviceToHost, side->stream));   // only the text comes back
    SPSP_HIP(hipStreamSynchronize(side->stream));          // the one wait
    return sg_collect_ms(side);
}

int windows_files(spsp_ctx* ctx, WindowsRun* run, const RecordsAsk& ask, double t_csv) {
    int rc;
    const auto taken = [](const std::string& s) { char* t = (char*)malloc(s.size() + 1); if (t) memcpy(t, s.c_str(), s.size() + 1); return t; };
    char* seg_text = taken(run->seg_csv);
    char* mos_text = taken(run->mos_csv);
    if (!seg_text || !mos_text) { free(seg_text); free(mos_text); set_error("out of host memory"); return SPSP_ERR_NOMEM; }
    if ((rc = write_csv_gz(ctx, seg_text, run->seg_csv.size(), ask.out_prefix, "_segments.csv.gz", t_csv))) { free(mos_text); return rc; }
    if ((rc = write_csv_gz(ctx, mos_text, run->mos_csv.size(), ask.out_prefix, "_mosaic.csv.gz", now_s()))) return rc;
    std::string path;
    if (run->want_fasta) {
        path = std::string(ask.out_prefix) + "_segments.fa" + (ask.gz ? ".gz" : "");
        const double t = now_s();
        rc = write_bytes(path.c_str(), run->fasta.data(), run->fasta.size(), ask.gz);
        ctx->stages.csv_gzip_s += now_s() - t;
        if (rc) return rc;
    }
    std::string bed_path;
    if (run->want_bed) {
        bed_path = std::string(ask.out_prefix) + "_segments.bed" + (ask.gz ? ".gz" : "");
        const double t = now_s();
        rc = write_bytes(bed_path.c_str(), reinterpret_cast<const uint8_t*>(run->bed.data()), run->bed.size(), ask.gz);
        ctx->stages.csv_gzip_s += now_s() - t;
        if (rc) return rc;
    }
    if (!ask.chatter) return SPSP_OK;
    const uint32_t n_rec = (uint32_t)(run->rec_off.size() - 1);
    uint64_t mixed = 0;
    for (const spsp_mosaic_row& m : run->mosaic) mixed += m.calls >= 2;
    printf("%u record(s) in %u window(s) of %llu base(s): %llu segment(s), %llu record(s) with two or more calls\n", n_rec, run->first_win[n_rec],
           (unsigned long long)run->window, (unsigned long long)run->segments.size(), (unsigned long long)mixed);
    if (ask.smooth) printf("smoothing at %u window(s): %llu window(s) took their neighbours' call\n", ask.smooth, (unsigned long long)run->n_changed);
    if (run->want_fasta)
        printf("segments %s: %llu of %llu segment(s) written, %llu base(s), %llu byte(s) to %s\n", ask.segments_what, (unsigned long long)run->n_written,
               (unsigned long long)run->segments.size(), (unsigned long long)run->bases_written, (unsigned long long)run->fasta.size(), path.c_str());
    if (run->want_bed)
        printf("raw coordinates: %llu segment(s) lifted, their raw intervals %llu base(s) longer than the kept ones, %llu byte(s) to %s\n", (unsigned long long)run->n_lifted,
               (unsigned long long)run->raw_excess, (unsigned long long)run->bed.size(), bed_path.c_str());
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_segments_write_device(spsp_ctx* ctx, const void* d_bases, uint64_t n_bases, int packed, const uint64_t* h_src, const uint64_t* h_len,
                                          const uint8_t* h_headers, const uint64_t* h_hdr_off, uint64_t n_seg, void** d_out, uint64_t* n_out) {
    if (!ctx || !d_out || !n_out || !h_hdr_off || (n_bases && !d_bases) || (n_seg && (!h_src || !h_len)) || (h_hdr_off[n_seg] != h_hdr_off[0] && !h_headers)) {
        set_error("NULL argument");
        return SPSP_ERR_ARG;
    }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint8_t* o = nullptr;
    const int rc = segments_write_impl(ctx, (const uint8_t*)d_bases, n_bases, packed != 0, h_src, h_len, h_headers, h_hdr_off, n_seg, &o, n_out);
    *d_out = o;
    return rc;
}

extern "C" int spsp_segments_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (const int rc = sg_collect_ms(ctx)) return rc;
    ms[0] = ctx->sg_ms; ctx->sg_ms = 0;
    return SPSP_OK;
}
