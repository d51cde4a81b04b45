// Windows on the GPU: every record of a cleaned text cut into overlapping windows, the windows' bases written back to back so that
// the scan, the key extraction and the record passes see windows as records (not in the reference, which has no record passes).
// The rule is in include/spsp.h ("windows"); this file is its device form.
//
// Counts, over tiles of 2 048 records (a lane walks eight):
//   k_wn_tiles    per tile the windows and the expanded bases of its records; offsets that decrease or leave the bases raise the flag
//   k_scan_items<WnSum>  one workgroup: the exclusive 64-bit scan of the tiles' two sums, and the totals (spsp_device.h)
//   k_wn_records  per tile: first_win[r] and the output start of every record, and the closing entries
// The host waits once, for the totals and first_win: they size everything behind.
//   k_wn_windows  a lane per WINDOW: its record by binary search over first_win, then its output offset and its source start.  A
//                 chromosome of 10^5 windows spreads over as many lanes; 10^6 reads of one window each cost a lane each.
// The copy (k_wn_copy_ascii, k_wn_copy_packed), the hot path, is balanced by OUTPUT: a workgroup owns 16 KiB of the output --
// 16 384 bases of ASCII, 65 536 bases of 2-bit words, whole dwords and whole 16-byte stores either way, so no store is shared
// between workgroups -- finds the windows that cross it with two binary searches over the new offsets, and every lane writes
// 16-byte-aligned 16-byte stores.  ASCII: a store inside one window takes two aligned 16-byte loads and a byte shift
// (ex_gather16); a store that straddles windows or the output's end is assembled byte by byte.  Packed: a lane makes the four
// dwords of its store; a dword takes the source dword that holds its first base and the next, funnel-shifted by twice the first
// base's place in its dword, and loops over the windows where it holds bases of several (W < 16, window and record ends).
// Stores behind the last base write zeros; the buffer is whole stretches and 256 cleared bytes: no store can leave it.
// Ordering is by the launches on the stream; no device-wide atomics but the flag's; plain vector stores.
#include <algorithm>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

enum WnWord { kWnBases = 0, kWnWins = 1, kWnBad = 2, kWnWords = 4 };   // the call's words on the device (64 bits each)
static_assert(kWnStores * kWnThreads * 16 == kWnStretchBytes && kWnStretchPacked % 64 == 0 && kWnStretch % 16 == 0, "a stretch is whole 16-byte stores");

// the records r0 .. r0 + 7 of one lane: their windows and expanded bases; on_rec(r, wins_before, bases_before) per record
template <class OnRec>
__device__ __forceinline__ void wn_walk(const uint64_t* __restrict__ off, uint32_t n_rec, uint64_t n_bases, uint64_t r0, uint32_t k, uint64_t S, WnSum& s, bool& bad,
                                        OnRec on_rec) {
    s = WnSum{0ull, 0ull};
    bad = false;
    if (r0 >= n_rec) return;
    uint64_t b0 = off[r0];
#pragma unroll
    for (uint32_t u = 0; u < kWnRecsPerLane; ++u) {
        const uint64_t r = r0 + u;
        if (r >= n_rec) break;
        const uint64_t b1 = off[r + 1];
        const bool ok = b0 <= b1 && b1 <= n_bases;
        if (!ok) bad = true;
        const uint64_t L = ok ? b1 - b0 : 0ull, n = wn_count(L, k, S);
        on_rec(r, s.wins, s.bases);
        s.wins += n;
        s.bases += wn_bases(L, n, k);
        b0 = b1;
    }
}

__global__ __launch_bounds__(kWnThreads) void k_wn_tiles(const uint64_t* __restrict__ off, uint32_t n_rec, uint64_t n_bases, uint32_t k, uint64_t S,
                                                         WnSum* __restrict__ tiles, unsigned long long* __restrict__ words) {
    __shared__ WnSum s_wave[kWnThreads / 64];
    WnSum s;
    bool bad;
    wn_walk(off, n_rec, n_bases, ((uint64_t)blockIdx.x * kWnThreads + threadIdx.x) * kWnRecsPerLane, k, S, s, bad, [](uint64_t, uint64_t, uint64_t) {});
    if (bad) atomicOr(words + kWnBad, 1ull);
    const WnSum all = block_sum<kWnThreads / 64>(s, s_wave);
    if (threadIdx.x == 0) tiles[blockIdx.x] = all;
}

// what the item scan does with a WnSum total
struct WnTotals {
    unsigned long long* words;
    __device__ void operator()(const WnSum& s) const { words[kWnBases] = s.bases; words[kWnWins] = s.wins; }
};

// rec_first[r], rec_out[r]: record r's first window and where its windows' bases begin in the output; [n_rec]: the totals
__global__ __launch_bounds__(kWnThreads) void k_wn_records(const uint64_t* __restrict__ off, uint32_t n_rec, uint64_t n_bases, uint32_t k, uint64_t S, uint64_t n_tiles,
                                                           const WnSum* __restrict__ base, const unsigned long long* __restrict__ words,
                                                           uint32_t* __restrict__ rec_first, uint64_t* __restrict__ rec_out) {
    __shared__ WnSum s_wave[kWnThreads / 64];
    const uint64_t r0 = ((uint64_t)blockIdx.x * kWnThreads + threadIdx.x) * kWnRecsPerLane;
    WnSum s;
    bool bad;
    wn_walk(off, n_rec, n_bases, r0, k, S, s, bad, [](uint64_t, uint64_t, uint64_t) {});
    const WnSum before = block_prefix_excl<kWnThreads / 64>(s, threadIdx.x & 63u, threadIdx.x >> 6, s_wave);
    if (blockIdx.x < n_tiles) {
        const unsigned long long a0 = base[blockIdx.x].bases + before.bases, b0 = base[blockIdx.x].wins + before.wins;
        WnSum again;
        wn_walk(off, n_rec, n_bases, r0, k, S, again, bad, [=](uint64_t r, uint64_t wins, uint64_t bases) { rec_first[r] = (uint32_t)(b0 + wins); rec_out[r] = a0 + bases; });
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec_first[n_rec] = (uint32_t)words[kWnWins]; rec_out[n_rec] = words[kWnBases]; }
}

// window w of all: win_off[w] = where its bases begin in the output, win_src[w] = where they begin in the source; [n_win]: the ends
__global__ __launch_bounds__(kWnThreads) void k_wn_windows(const uint64_t* __restrict__ off, uint32_t n_rec, const uint32_t* __restrict__ rec_first,
                                                           const uint64_t* __restrict__ rec_out, uint64_t window, uint64_t S, uint32_t n_win, uint64_t n_bases,
                                                           uint64_t* __restrict__ win_off, uint64_t* __restrict__ win_src) {
    const uint64_t w = (uint64_t)blockIdx.x * kWnThreads + threadIdx.x;
    if (w > n_win) return;
    if (w == n_win) { win_off[w] = rec_out[n_rec]; win_src[w] = n_bases; return; }
    uint32_t lo = 0, hi = n_rec;                           // (every record has a window: first_win ascends strictly, and rec_first[0] = 0 <= w)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rec_first[mid] <= w) lo = mid; else hi = mid;
    }
    const uint64_t i = w - rec_first[lo];
    win_off[w] = rec_out[lo] + i * window;                 // (every window in front of it in the record has W bases)
    win_src[w] = off[lo] + i * S;
}

__global__ __launch_bounds__(kWnThreads) void k_wn_copy_ascii(const uint8_t* __restrict__ bases, uint64_t n_bases, const uint64_t* __restrict__ win_off,
                                                              const uint64_t* __restrict__ win_src, uint32_t n_win, uint64_t n_out, uint8_t* __restrict__ out) {
    __shared__ uint32_t s_range[2];
    const uint64_t o_wg = (uint64_t)blockIdx.x * kWnStretch;
    const bool any = o_wg < n_out && n_win != 0u;          // (uniform.  The grid's last stretch may lie behind the last base: it is zeros)
    if (any) {
        if (threadIdx.x == 0u) s_range[0] = ex_find(win_off, 0u, n_win, o_wg);
        if (threadIdx.x == 64u) s_range[1] = ex_find(win_off, 0u, n_win, (o_wg + kWnStretch < n_out ? o_wg + kWnStretch : n_out) - 1ull);
    }
    __syncthreads();
    const uint32_t i_lo = any ? s_range[0] : 0u, i_hi = any ? s_range[1] + 1u : 0u;
#pragma unroll
    for (uint32_t it = 0; it < kWnStores; ++it) {
        const uint64_t o = o_wg + (uint64_t)(it * kWnThreads + threadIdx.x) * 16ull;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (o < n_out) {
            uint32_t i = ex_find(win_off, i_lo, i_hi, o);
            uint64_t rd = win_off[i], re = win_off[i + 1], rs = win_src[i];
            if (o + 16ull <= re && rs + (o - rd) + 16ull <= n_bases) {
                v = ex_gather16(bases, n_bases, rs + (o - rd));   // inside one window: the two aligned groups that hold the 16 source bytes
            } else {
                // across windows or the output's end: byte by byte (zeros behind the end)
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t b = 0; b < 16u; ++b) {
                    const uint64_t pos = o + b;
                    if (pos < n_out) {
                        while (pos >= re) { ++i; rs = win_src[i]; rd = re; re = win_off[i + 1]; }   // (win_off[n_win] = n_out: i stays below n_win)
                        const uint64_t s = rs + (pos - rd);
                        w[b >> 2] |= (s < n_bases ? (uint32_t)bases[s] : 0u) << (8 * (b & 3u));
                    }
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        *reinterpret_cast<uint4*>(out + o) = v;
    }
}

// the `take` bases from base s on, in the top bits of a word: the dword that holds base s and, where they reach into it, the next,
// funnel-shifted by twice s's place in its dword.  n_words: the dwords that hold bases
__device__ __forceinline__ uint32_t wn_fetch(const uint32_t* __restrict__ src, uint64_t n_words, uint64_t s, uint32_t take) {
    const uint64_t q = s >> 4;
    const uint32_t at = (uint32_t)(s & 15ull), sh = 2u * at;
    const uint32_t hi = q < n_words ? src[q] : 0u;
    if (sh == 0u) return hi;
    const uint32_t lo = at + take > 16u && q + 1 < n_words ? src[q + 1] : 0u;
    return (hi << sh) | (lo >> (32u - sh));                // (one v_alignbit_b32)
}

__global__ __launch_bounds__(kWnThreads) void k_wn_copy_packed(const uint32_t* __restrict__ src, uint64_t n_bases, const uint64_t* __restrict__ win_off,
                                                               const uint64_t* __restrict__ win_src, uint32_t n_win, uint64_t n_out, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_range[2];
    const uint64_t o_wg = (uint64_t)blockIdx.x * kWnStretchPacked, n_words = (n_bases + 15ull) >> 4;
    const bool any = o_wg < n_out && n_win != 0u;          // (uniform)
    if (any) {
        if (threadIdx.x == 0u) s_range[0] = ex_find(win_off, 0u, n_win, o_wg);
        if (threadIdx.x == 64u) s_range[1] = ex_find(win_off, 0u, n_win, (o_wg + kWnStretchPacked < n_out ? o_wg + kWnStretchPacked : n_out) - 1ull);
    }
    __syncthreads();
    const uint32_t i_lo = any ? s_range[0] : 0u, i_hi = any ? s_range[1] + 1u : 0u;
#pragma unroll
    for (uint32_t it = 0; it < kWnStores; ++it) {
        const uint64_t o = o_wg + (uint64_t)(it * kWnThreads + threadIdx.x) * 64ull;   // the first base of this lane's four dwords
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (o < n_out) {
            uint32_t i = ex_find(win_off, i_lo, i_hi, o);
            uint64_t rd = win_off[i], re = win_off[i + 1], rs = win_src[i];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint64_t p = o + 16ull * j;
                uint32_t word = 0u;
                for (uint32_t b = 0; b < 16u && p + b < n_out;) {   // one trip inside a window; more where the dword holds several windows' bases
                    const uint64_t pos = p + b;
                    while (pos >= re) { ++i; rs = win_src[i]; rd = re; re = win_off[i + 1]; }   // (win_off[n_win] = n_out: i stays below n_win)
                    const uint32_t take = re - pos < (uint64_t)(16u - b) ? (uint32_t)(re - pos) : 16u - b;
                    uint32_t x = wn_fetch(src, n_words, rs + (pos - rd), take);
                    if (take < 16u) x &= ~(0xffffffffu >> (2u * take));
                    word |= x >> (2u * b);
                    b += take;
                }
                v[j] = word;
            }
        }
        *reinterpret_cast<uint4*>(out + (o >> 4)) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

int wn_mark(spsp_ctx* ctx, int i) {
    if (!ctx->timing) return SPSP_OK;
    if (!ctx->wn_ev[i]) SPSP_HIP(hipEventCreate(&ctx->wn_ev[i]));
    SPSP_HIP(hipEventRecord(ctx->wn_ev[i], ctx->stream));
    return SPSP_OK;
}

}  // namespace

int records_windows_impl(spsp_ctx* ctx, const uint8_t* d_bases, uint64_t n_bases, const uint64_t* d_rec_off, uint32_t n_rec, uint32_t k, uint64_t window, bool packed,
                         uint8_t** d_out, uint64_t* n_out, uint64_t** d_win_off, uint32_t* h_first_win, uint64_t* n_windows) {
    int rc;
    *d_out = nullptr; *n_out = 0; *d_win_off = nullptr; *n_windows = 0;
    for (uint64_t r = 0; r <= n_rec; ++r) h_first_win[r] = 0;
    if (k == 0 || window < k || window > kWnMaxWidth) {
        set_error("windows: the width must be k .. %llu (k = %u, width = %llu)", (unsigned long long)kWnMaxWidth, k, (unsigned long long)window);
        return SPSP_ERR_ARG;
    }
    if (n_rec > 0xfffffff0u) { set_error("too many records for one call (%u)", n_rec); return SPSP_ERR_OVERFLOW; }
    if (((uintptr_t)d_bases & 15u) != 0) { set_error("d_bases must be 16-byte aligned"); return SPSP_ERR_ARG; }
    const uint64_t S = window - (k - 1), n_rtiles = ((uint64_t)n_rec + kWnRecTile - 1) / kWnRecTile;
    if ((rc = ctx->wn_words.reserve(kWnWords * 8)) || (rc = ctx->wn_tiles.reserve((size_t)(n_rtiles + 1) * 2 * sizeof(WnSum))) ||
        (rc = ctx->wn_rec.reserve(((size_t)n_rec + 1) * 12 + 16))) return rc;
    unsigned long long* words = ctx->wn_words.as<unsigned long long>();
    WnSum* tiles = ctx->wn_tiles.as<WnSum>();
    WnSum* base = tiles + (n_rtiles + 1);
    uint64_t* rec_out = ctx->wn_rec.as<uint64_t>();
    uint32_t* rec_first = reinterpret_cast<uint32_t*>(rec_out + ((size_t)n_rec + 1));
    SPSP_HIP(hipMemsetAsync(words, 0, kWnWords * 8, ctx->stream));
    if ((rc = wn_mark(ctx, 0))) return rc;
    if (n_rtiles) hipLaunchKernelGGL(k_wn_tiles, dim3((uint32_t)n_rtiles), dim3(kWnThreads), 0, ctx->stream, d_rec_off, n_rec, n_bases, k, S, tiles, words);
    hipLaunchKernelGGL((k_scan_items<WnSum, WnTotals>), dim3(1), dim3(1024), 0, ctx->stream, (const WnSum*)tiles, n_rtiles, base, WnTotals{words});
    hipLaunchKernelGGL(k_wn_records, dim3((uint32_t)std::max<uint64_t>(n_rtiles, 1)), dim3(kWnThreads), 0, ctx->stream, d_rec_off, n_rec, n_bases, k, S, n_rtiles,
                       (const WnSum*)base, (const unsigned long long*)words, rec_first, rec_out);
    SPSP_HIP(hipGetLastError());
    uint64_t h[kWnWords];
    SPSP_HIP(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(h_first_win, rec_first, ((size_t)n_rec + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait: the counts size what follows
    const auto refuse = [&](int code) { for (uint64_t r = 0; r <= n_rec; ++r) h_first_win[r] = 0; return code; };
    if (h[kWnBad]) { set_error("windows: the record offsets must not decrease and must end inside the bases"); return refuse(SPSP_ERR_ARG); }
    if (h[kWnWins] > kWnMaxWindows) {
        set_error("windows: %llu windows, more than %llu: a wider window, or fewer records per call", (unsigned long long)h[kWnWins], (unsigned long long)kWnMaxWindows);
        return refuse(SPSP_ERR_OVERFLOW);
    }
    const uint64_t total = h[kWnBases];
    const uint32_t n_win = (uint32_t)h[kWnWins];
    const uint64_t stretch = packed ? kWnStretchPacked : kWnStretch;
    const uint64_t grid = std::max<uint64_t>((total + stretch - 1) / stretch, 1);
    if (grid > 0x7fffffffull) { set_error("windows: %llu bases of windows are too many for one call", (unsigned long long)total); return refuse(SPSP_ERR_OVERFLOW); }
    const size_t out_bytes = (size_t)grid * kWnStretchBytes;
    if ((rc = ctx->wn_off.reserve(((size_t)n_win + 1) * 8)) || (rc = ctx->wn_src.reserve(((size_t)n_win + 1) * 8)) || (rc = ctx->wn_out.reserve(out_bytes + kWnHalo)))
        return refuse(rc);
    uint64_t* win_off = ctx->wn_off.as<uint64_t>();
    uint64_t* win_src = ctx->wn_src.as<uint64_t>();
    if ((rc = wn_mark(ctx, 1))) return rc;
    hipLaunchKernelGGL(k_wn_windows, dim3((uint32_t)(((uint64_t)n_win + 1 + kWnThreads - 1) / kWnThreads)), dim3(kWnThreads), 0, ctx->stream, d_rec_off, n_rec,
                       (const uint32_t*)rec_first, (const uint64_t*)rec_out, window, S, n_win, n_bases, win_off, win_src);
    SPSP_HIP(hipGetLastError());
    if ((rc = wn_mark(ctx, 2))) return rc;
    SPSP_HIP(hipMemsetAsync(ctx->wn_out.as<uint8_t>() + out_bytes, 0, kWnHalo, ctx->stream));
    if (packed) hipLaunchKernelGGL(k_wn_copy_packed, dim3((uint32_t)grid), dim3(kWnThreads), 0, ctx->stream, reinterpret_cast<const uint32_t*>(d_bases), n_bases,
                                   (const uint64_t*)win_off, (const uint64_t*)win_src, n_win, total, ctx->wn_out.as<uint32_t>());
    else hipLaunchKernelGGL(k_wn_copy_ascii, dim3((uint32_t)grid), dim3(kWnThreads), 0, ctx->stream, d_bases, n_bases, (const uint64_t*)win_off,
                            (const uint64_t*)win_src, n_win, total, ctx->wn_out.as<uint8_t>());
    SPSP_HIP(hipGetLastError());
    if ((rc = wn_mark(ctx, 3))) return rc;
    if (ctx->timing) {                                     // (only then: the spans are read behind the copy)
        SPSP_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < 3; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ctx->wn_ev[i], ctx->wn_ev[i + 1])); ctx->wn_ms[i] += ms; }
    }
    *d_out = ctx->wn_out.as<uint8_t>(); *n_out = total; *d_win_off = win_off; *n_windows = n_win;
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_records_windows_device(spsp_ctx* ctx, const void* d_bases, uint64_t n_bases, const void* d_rec_off, uint32_t n_rec, uint32_t k, uint64_t window,
                                           int packed, void** d_out, uint64_t* n_out, void** d_win_off, uint32_t* h_first_win, uint64_t* n_windows) {
    if (!ctx || !d_out || !n_out || !d_win_off || !h_first_win || !n_windows || !d_rec_off || (n_bases && !d_bases)) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint8_t* o = nullptr; uint64_t* w = nullptr;
    const int rc = records_windows_impl(ctx, (const uint8_t*)d_bases, n_bases, (const uint64_t*)d_rec_off, n_rec, k, window, packed != 0, &o, n_out, &w, h_first_win,
                                        n_windows);
    *d_out = o; *d_win_off = w;
    return rc;
}

extern "C" int spsp_windows_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (int i = 0; i < 3; ++i) { ms[i] = ctx->wn_ms[i]; ctx->wn_ms[i] = 0; }
    return SPSP_OK;
}
