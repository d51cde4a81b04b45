// Downsampling of comparator keys on the GPU: a sketch made at rate s holds every coarser sketch of the same genome.
//
// A k-mer is selected iff XXH64 (seed 1312) of its canonical minimizer is <= threshold(k, m, s) and nothing else in the
// scan depends on the threshold, so   keys(sketch(G, s')) = { (min, kmer) in keys(sketch(G, s)) : xxh64(min) <= T(s') }
// for s' >= s: a streaming compaction of the concatenated key arrays, order kept.
//
// One fixed chain of launches whatever the number of sketches is -- the keys are cut into tiles of 2048, not into sketches:
//   k_ds_flag     one workgroup per tile: 4 B read per key, one hash, a wave ballot -> one 64-bit word of keep bits per 64
//                 keys and the tile's survivor count
//   scan          launch_scan_u32 over the tile counts -> where every tile's survivors go
//   k_ds_move     one workgroup per tile: the tile's 32 ballot words -> a prefix per word; lane l of a kept key writes at
//                 tile offset + word prefix + popcount(word below l): neighbouring survivors land side by side
//   k_ds_offsets  one thread per sketch boundary: survivors in front of it = its tile's offset + the bits in front of it
// and ONE host wait, the one that reads the new offsets back.  No host path.  Everything behind the flags is ds_compact_launch
// (spsp_internal.h).  The selection (spsp_select.hip) and the groups pass (spsp_groups.hip) keep by a word per entry instead of a hash:
// k_ds_flag_band makes their keep mask in the same layout and ds_flag_compact_launch runs it in front of the same three launches.
#include <algorithm>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

// round r of wave w of tile t fills word 32 t + 4 r + w of the keep mask: bit l of word j is key 64 j + l
__global__ __launch_bounds__(kDsThreads) void k_ds_flag(const uint32_t* __restrict__ mn, uint32_t n_keys, uint64_t threshold,
                                                        unsigned long long* __restrict__ mask, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_cnt[kDsThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * kDsTile + threadIdx.x;       // (n_keys <= 0xfffffff0 and the last tile starts below it)
    uint32_t v[kDsTile / kDsThreads];
#pragma unroll
    for (uint32_t r = 0; r < kDsTile / kDsThreads; ++r) {
        const uint64_t i = (uint64_t)base + r * kDsThreads;
        v[r] = i < n_keys ? mn[i] : 0u;
    }
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kDsTile / kDsThreads; ++r) {
        const uint64_t i = (uint64_t)base + r * kDsThreads;
        const bool keep = i < n_keys && xxh64_u64((uint64_t)v[r]) <= threshold;
        const unsigned long long word = __ballot(keep);
        if (lane == 0) mask[(size_t)blockIdx.x * kDsWords + r * (kDsThreads / 64) + w] = word;
        cnt += (uint32_t)__popcll(word);
    }
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// keep bit of entry i of [0, n_keys): every bit of `need` set in value[i], and value[i]'s low 31 bits in [h_min, h_max].  The
// selection: value = holders[] (need = 0x80000000 for the merged form -- only the entry that claimed its key's slot speaks for the
// key -- else 0).  Round r of wave w of tile t fills word 32 t + 4 r + w (k_ds_flag's layout)
__global__ __launch_bounds__(kDsThreads) void k_ds_flag_band(const uint32_t* __restrict__ holders, uint32_t n_keys, uint32_t h_min, uint32_t h_max,
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

template <bool HAS_HI>
__global__ __launch_bounds__(kDsThreads) void k_ds_move(const uint32_t* __restrict__ mn, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi,
                                                        const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ tile_off,
                                                        uint32_t* __restrict__ out_mn, uint64_t* __restrict__ out_lo, uint64_t* __restrict__ out_hi) {
    __shared__ unsigned long long s_word[kDsWords];
    __shared__ uint32_t s_pre[kDsWords];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (threadIdx.x < 64) {
        // the tile's 32 words, in key order, and how many survivors lie in front of each
        const unsigned long long word = lane < kDsWords ? mask[(size_t)blockIdx.x * kDsWords + lane] : 0ull;
        const uint32_t c = (uint32_t)__popcll(word);
        uint32_t x = c;
#pragma unroll
        for (int d = 1; d < (int)kDsWords; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (lane >= (uint32_t)d) x += y; }
        if (lane < kDsWords) { s_word[lane] = word; s_pre[lane] = x - c; }
    }
    __syncthreads();
    const uint32_t at = tile_off[blockIdx.x];
    const uint32_t base = blockIdx.x * kDsTile + threadIdx.x;
#pragma unroll
    for (uint32_t r = 0; r < kDsTile / kDsThreads; ++r) {
        const uint32_t wi = r * (kDsThreads / 64) + w;
        const unsigned long long word = s_word[wi];
        if (!((word >> lane) & 1ull)) continue;                      // (a set bit is a key inside the arrays: k_ds_flag)
        const uint64_t i = (uint64_t)base + r * kDsThreads;
        const uint32_t dst = at + s_pre[wi] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        out_mn[dst] = mn[i];
        out_lo[dst] = lo[i];
        if (HAS_HI) out_hi[dst] = hi[i];
    }
}

// off_out[i] = survivors among the keys in front of off_in[i] (offsets relative to the first sketch's first key)
__global__ __launch_bounds__(256) void k_ds_offsets(const uint64_t* __restrict__ off_in, uint32_t n_bounds, uint32_t n_tiles,
                                                    const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ tile_off,
                                                    uint64_t* __restrict__ off_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_bounds) return;
    const uint64_t pos = off_in[i];
    const uint64_t t = pos / kDsTile;
    uint32_t c = tile_off[t < n_tiles ? t : n_tiles];                // (tile_off has n_tiles + 1 entries: the last is the total)
    if (t < n_tiles) {
        const uint64_t w_end = pos >> 6;
        for (uint64_t wd = t * kDsWords; wd < w_end; ++wd) c += (uint32_t)__popcll(mask[wd]);
        if (pos & 63u) c += (uint32_t)__popcll(mask[w_end] & ((1ull << (pos & 63u)) - 1ull));
    }
    off_out[i] = c;
}

}  // namespace

// (spsp_internal.h) scan, move, offsets: what follows a keep mask, whoever made it
int ds_compact_launch(spsp_ctx* ctx, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const unsigned long long* d_mask,
                      const uint32_t* d_tile_cnt, uint32_t* d_tile_off, uint32_t n_tiles, const uint64_t* d_off_in, uint32_t n_bounds, uint64_t* d_off_out,
                      uint32_t* out_mn, uint64_t* out_lo, uint64_t* out_hi, uint64_t* total_host) {
    int rc;
    if ((rc = launch_scan_u32(ctx, d_tile_cnt, d_tile_off, n_tiles, total_host))) return rc;
    if (has_hi) hipLaunchKernelGGL(k_ds_move<true>, dim3(n_tiles), dim3(kDsThreads), 0, ctx->stream, d_mn, d_lo, d_hi, d_mask, (const uint32_t*)d_tile_off,
                                   out_mn, out_lo, out_hi);
    else hipLaunchKernelGGL(k_ds_move<false>, dim3(n_tiles), dim3(kDsThreads), 0, ctx->stream, d_mn, d_lo, (const uint64_t*)nullptr, d_mask,
                            (const uint32_t*)d_tile_off, out_mn, out_lo, (uint64_t*)nullptr);
    hipLaunchKernelGGL(k_ds_offsets, dim3((n_bounds + 255) / 256), dim3(256), 0, ctx->stream, d_off_in, n_bounds, n_tiles, d_mask, (const uint32_t*)d_tile_off,
                       d_off_out);
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

// (spsp_internal.h) offsets up, k_ds_flag_band, ds_compact_launch, offsets down.  h_rel and h_off_out stay the caller's until its wait
int ds_flag_compact_launch(spsp_ctx* ctx, const DsWork& W, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint32_t* d_value,
                           uint32_t n_keys, uint32_t h_min, uint32_t h_max, uint32_t need, const uint64_t* h_rel, uint32_t n_bounds, uint32_t* out_mn,
                           uint64_t* out_lo, uint64_t* out_hi, uint64_t* total_host, uint64_t* h_off_out) {
    int rc;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n_keys + kDsTile - 1) / kDsTile);
    SPSP_HIP(hipMemcpyAsync(W.off_in, h_rel, (size_t)n_bounds * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ds_flag_band, dim3(n_tiles), dim3(kDsThreads), 0, ctx->stream, d_value, n_keys, h_min, h_max, need, W.mask, W.tile_cnt);
    SPSP_HIP(hipGetLastError());
    if ((rc = ds_compact_launch(ctx, has_hi, d_mn, d_lo, d_hi, W.mask, W.tile_cnt, W.tile_off, n_tiles, W.off_in, n_bounds, W.off_out, out_mn,
                                out_lo, out_hi, total_host))) return rc;
    SPSP_HIP(hipMemcpyAsync(h_off_out, W.off_out, (size_t)n_bounds * 8, hipMemcpyDeviceToHost, ctx->stream));
    return SPSP_OK;
}

int keys_downsample_impl(spsp_ctx* ctx, uint32_t k, uint64_t threshold, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi,
                         const uint64_t* h_sk_off, uint32_t n, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi, uint64_t* sk_off_out) {
    const bool has_hi = k > 32;
    for (uint32_t i = 0; i < n; ++i)
        if (h_sk_off[i + 1] < h_sk_off[i]) { set_error("sketch offsets must not decrease (sketch %u)", i); return SPSP_ERR_ARG; }
    const uint64_t first = h_sk_off[0], R = h_sk_off[n] - first;
    if (R > 0xfffffff0ull) { set_error("too many sketch k-mers for one call"); return SPSP_ERR_OVERFLOW; }
    if (R && (!d_mn || !d_lo || (has_hi && !d_hi))) { set_error("NULL key array"); return SPSP_ERR_ARG; }
    // two sets of output arrays, used in turn: the result of one call may be the input of the next (10 -> 100 -> 1000)
    const int set = ctx->ds_flip;
    ctx->ds_flip ^= 1;
    int rc;
    if ((rc = ctx->ds_mn[set].reserve((size_t)R * 4 + 64)) || (rc = ctx->ds_lo[set].reserve((size_t)R * 8 + 64)) ||
        (has_hi && (rc = ctx->ds_hi[set].reserve((size_t)R * 8 + 64)))) return rc;
    *out_mn = ctx->ds_mn[set].as<uint32_t>(); *out_lo = ctx->ds_lo[set].as<uint64_t>(); *out_hi = has_hi ? ctx->ds_hi[set].as<uint64_t>() : nullptr;
    for (uint32_t i = 0; i <= n; ++i) sk_off_out[i] = 0;
    if (R == 0) return SPSP_OK;
    d_mn += first; d_lo += first; if (has_hi) d_hi += first;
    const uint32_t n_tiles = (uint32_t)((R + kDsTile - 1) / kDsTile);
    const size_t off_bytes = ((size_t)n + 1) * 8;
    if ((rc = ctx->ds_work.reserve(DsWork::bytes(n_tiles, n + 1)))) return rc;
    const DsWork W(ctx->ds_work.p, n_tiles, n + 1);
    std::vector<uint64_t> rel((size_t)n + 1);
    for (uint32_t i = 0; i <= n; ++i) rel[i] = h_sk_off[i] - first;
    SPSP_HIP(hipMemcpyAsync(W.off_in, rel.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ds_flag, dim3(n_tiles), dim3(kDsThreads), 0, ctx->stream, d_mn, (uint32_t)R, threshold, W.mask, W.tile_cnt);
    SPSP_HIP(hipGetLastError());
    if ((rc = ds_compact_launch(ctx, has_hi, d_mn, d_lo, d_hi, W.mask, W.tile_cnt, W.tile_off, n_tiles, W.off_in, n + 1, W.off_out, *out_mn, *out_lo, *out_hi,
                                ctx->h_scalar + kHsDownsampleTotal))) return rc;
    SPSP_HIP(hipMemcpyAsync(sk_off_out, W.off_out, off_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));                    // (the one wait; `rel` has been read by then)
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_keys_downsample_device(spsp_ctx* ctx, uint32_t k, uint64_t threshold, const void* d_minimizer, const void* d_kmer_lo,
                                           const void* d_kmer_hi, const uint64_t* h_sk_off, uint32_t n, void** d_out_minimizer, void** d_out_kmer_lo,
                                           void** d_out_kmer_hi, uint64_t* sk_off_out) {
    if (!ctx || !h_sk_off || !d_out_minimizer || !d_out_kmer_lo || !d_out_kmer_hi || !sk_off_out) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (k < 1 || k > 63) { set_error("k=%u out of range 1..63", k); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint32_t* mn = nullptr; uint64_t *lo = nullptr, *hi = nullptr;
    const int rc = keys_downsample_impl(ctx, k, threshold, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n,
                                        &mn, &lo, &hi, sk_off_out);
    if (rc) return rc;
    *d_out_minimizer = mn; *d_out_kmer_lo = lo; *d_out_kmer_hi = hi;
    return SPSP_OK;
}
