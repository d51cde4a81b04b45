// Prevalence on the GPU: how many of the references hold each key, and what follows from that one number per key -- the core,
// shell and unique keys of every row sketch, and the spectrum of the references' union (not in the reference, whose end product
// is the two n x n matrices).
//
// Keys are the comparator's: the distinct (minimizer, canonical k-mer) pairs of a sketch, sorted by (minimizer, kmer_hi,
// kmer_lo), the sketches back to back.  n_query == 0: every sketch is a row and a reference (R = n); n_query > 0: the first
// n_query sketches are rows only, the R = n - n_query behind them the references.  h(x) = the references that hold key x.
// Classes of a key, in this order: absent (h == 0), core (h * den >= num * R), unique (h == 1), shell.  Integers only.
//
// A key arrives with ALL its holders -- 65 535 copies of one genome are 65 535 entries of every key -- so nothing here keeps a
// key's records in LDS (that form has its cliff exactly where this result is wanted most).  One table in HBM:
//   k_pv_count     a lane per REFERENCE entry: its key's slot -- the first free slot of the probe sequence, claimed by a CAS of
//                  the entry's number, or the slot whose claimer holds the same FULL key (read through the claimer's entry: no
//                  fingerprint, nothing to collide) -- and one atomic add on the slot's counter.  Claimer and counter are the
//                  two halves of one 64-bit word: a probe reads one line.  Queries never insert.
//   k_pv_read      a lane per entry, references and queries alike: the same probe sequence without the claim; holders[e] = the
//                  slot's counter, 0 for a query key that meets a free slot.  The store is coalesced.
//   k_pv_rows      a workgroup per row sketch over its slice of holders[]: the four classes and the sum of h by wave
//                  reductions, no global atomic.
//   k_pv_spectrum  lanes over the table's slots: LDS bins over a window of 8 192 holder counts per blockIdx.y; a wave whose
//                  claimed slots all carry one count adds once (one species: every key sits in bin R); the non-zero bins are
//                  flushed once per workgroup.
// The table's size follows from the number of reference entries alone, so no attempt is ever repeated, and the host waits
// once, at the end.  No workgroup ever waits for another one: the order is the order of the launches on the stream.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kPvThreads = 256;                       // 4 waves, every kernel
constexpr uint32_t kPvWindow = 8192;                       // k_pv_spectrum: bins per workgroup (32 KiB of LDS)
constexpr uint32_t kPvSpecBlocksPerCu = 4;
constexpr uint32_t kPvMaxDen = 1000000;
constexpr uint32_t kPvLog2CapMax = 32;                     // (an entry's number + 1 is a 32-bit word: never more entries than that)
enum { kPvwBad = 0, kPvwWrapped = 1, kPvWords = 4 };       // flag words in front of the spectrum (16 bytes, cleared with it)

// (pv_home, pv_same: spsp_device.h)
// a slot word: the claimer's entry number + 1 in the low half (0: free), the holders counted so far in the high half
template <bool HAS_HI>
__global__ __launch_bounds__(kPvThreads) void k_pv_count(SortedKeys K, const uint64_t* __restrict__ off, uint32_t n, uint32_t nq,
                                                         unsigned long long* __restrict__ tbl, uint32_t log2cap, uint32_t* __restrict__ words) {
    const uint64_t e = off[nq] + (uint64_t)blockIdx.x * kPvThreads + threadIdx.x;
    if (e >= off[n]) return;
    const uint32_t mn = K.mn[e];
    const uint64_t lo = K.lo[e], hi = HAS_HI ? K.hi[e] : 0ull;
    sorted_check_order<HAS_HI>(K, off, nq, n, e, mn, hi, lo, words + kPvwBad);
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t pos = pv_home<HAS_HI>(mn, hi, lo, log2cap);
    for (uint64_t probes = 0;; ++probes) {
        // (a stale 0 from this CU's L1 only costs the CAS, which answers with the word as it is; a claim never changes)
        unsigned long long cur = tbl[pos];
        if ((uint32_t)cur == 0u) cur = atomicCAS(&tbl[pos], 0ull, (unsigned long long)((uint32_t)e + 1u));
        if ((uint32_t)cur == 0u) break;                    // claimed
        if (pv_same<HAS_HI>(K, (uint64_t)((uint32_t)cur - 1u), mn, hi, lo)) break;
        // (never: the table has a slot per reference entry at the least and an entry claims one slot at the most.  The bound keeps a
        // lane from going round whatever a caller's arrays hold)
        if (probes >= mask) { atomicOr(words + kPvwWrapped, 1u); return; }
        pos = (pos + 1ull) & mask;
    }
    atomicAdd(&tbl[pos], 1ull << 32);                      // (result unused: a key of one species puts R of these on one word)
}

// CLAIM (the selection's merged form): bit 31 of holders[e] says that e is the entry whose number the slot's low half names
template <bool HAS_HI, bool CLAIM>
__global__ __launch_bounds__(kPvThreads) void k_pv_read(SortedKeys K, const uint64_t* __restrict__ off, uint32_t n, uint32_t nq,
                                                        const unsigned long long* __restrict__ tbl, uint32_t log2cap, uint32_t* __restrict__ holders,
                                                        uint32_t* __restrict__ words) {
    const uint64_t e = off[0] + (uint64_t)blockIdx.x * kPvThreads + threadIdx.x;
    if (e >= off[n]) return;
    const uint32_t mn = K.mn[e];
    const uint64_t lo = K.lo[e], hi = HAS_HI ? K.hi[e] : 0ull;
    if (e < off[nq]) sorted_check_order<HAS_HI>(K, off, 0, nq, e, mn, hi, lo, words + kPvwBad);   // (the references': k_pv_count)
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t pos = pv_home<HAS_HI>(mn, hi, lo, log2cap);
    uint32_t h = 0;
    for (uint64_t probes = 0; probes <= mask; ++probes) {  // (a query key may go round a table without a free slot: h stays 0)
        const unsigned long long cur = tbl[pos];
        if ((uint32_t)cur == 0u) break;
        if (pv_same<HAS_HI>(K, (uint64_t)((uint32_t)cur - 1u), mn, hi, lo)) {
            h = (uint32_t)(cur >> 32);
            if (CLAIM && (uint32_t)cur - 1u == (uint32_t)e) h |= 0x80000000u;   // (a counter is 65 535 at the most)
            break;
        }
        pos = (pos + 1ull) & mask;
    }
    holders[e] = h;
}

// one workgroup per row sketch; core_min = the least h that is core: ceil(num * R / den) >= 1
__global__ __launch_bounds__(kPvThreads) void k_pv_rows(const uint32_t* __restrict__ holders, const uint64_t* __restrict__ off, uint32_t core_min,
                                                        spsp_prevalence_row* __restrict__ rows) {
    __shared__ unsigned long long s_part[kPvThreads / 64][5];
    const uint32_t i = blockIdx.x, t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    const uint64_t end = off[i + 1];
    uint32_t core = 0, shell = 0, uniq = 0, absent = 0;    // (per lane: fewer than 2^32 entries in all)
    unsigned long long held = 0;
    for (uint64_t e = off[i] + t; e < end; e += kPvThreads) {
        const uint32_t h = holders[e];
        held += h;
        if (h == 0u) ++absent;
        else if (h >= core_min) ++core;
        else if (h == 1u) ++uniq;
        else ++shell;
    }
    unsigned long long v[5] = {core, shell, uniq, absent, held};
#pragma unroll
    for (int f = 0; f < 5; ++f) {
#pragma unroll
        for (int d = 32; d; d >>= 1) v[f] += __shfl_down(v[f], d);
        if (lane == 0) s_part[wid][f] = v[f];
    }
    __syncthreads();
    if (t != 0) return;
    unsigned long long s[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        s[f] = 0;
#pragma unroll
        for (uint32_t w = 0; w < kPvThreads / 64; ++w) s[f] += s_part[w][f];
    }
    spsp_prevalence_row r;
    r.core = s[0]; r.shell = s[1]; r.unique = s[2]; r.absent = s[3]; r.holders = s[4];
    rows[i] = r;
}

// grid.x = shares of the table's slots (grid-stride), grid.y = window of kPvWindow holder counts; spectrum[t] for t <= R only
__global__ __launch_bounds__(kPvThreads) void k_pv_spectrum(const unsigned long long* __restrict__ tbl, uint64_t cap, uint32_t R,
                                                            unsigned long long* __restrict__ spectrum) {
    __shared__ uint32_t s_bin[kPvWindow];                  // (a workgroup sees fewer than 2^32 slots)
    const uint32_t first = blockIdx.y * kPvWindow, lane = threadIdx.x & 63u;
    for (uint32_t b = threadIdx.x; b < kPvWindow; b += kPvThreads) s_bin[b] = 0u;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * kPvThreads; base < cap; base += (uint64_t)gridDim.x * kPvThreads) {   // (uniform: no lane leaves early)
        const uint64_t s = base + threadIdx.x;
        uint32_t b = 0;
        bool in = false;
        if (s < cap) {
            const unsigned long long w = tbl[s];
            if ((uint32_t)w != 0u) { b = (uint32_t)(w >> 32) - first; in = b < kPvWindow; }   // (a count below the window wraps beyond it)
        }
        const unsigned long long word = __ballot(in);
        if (word == 0ull) continue;
        const int leader = __ffsll((long long)word) - 1;
        const uint32_t b0 = __shfl(b, leader);
        if (__ballot(in && b != b0) == 0ull) {             // one count in the whole wave: one add
            if ((int)lane == leader) atomicAdd(&s_bin[b0], (uint32_t)__popcll(word));
        } else if (in) atomicAdd(&s_bin[b], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kPvWindow; b += kPvThreads) {
        const uint32_t c = s_bin[b];
        if (c != 0u && first + b <= R) atomicAdd(&spectrum[first + b], (unsigned long long)c);
    }
}

}  // namespace

int prevalence_check_args(uint32_t n, uint32_t n_query, uint32_t num, uint32_t den) {
    if (n == 0 || n > 65535) { set_error("prevalence takes 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    if (n_query >= n) { set_error("prevalence: %u queries of %u sketches (0: all versus all; else at least one reference behind them)", n_query, n); return SPSP_ERR_ARG; }
    if (num == 0 || num > den || den > kPvMaxDen) { set_error("prevalence threshold %u / %u: needs 1 <= num <= den <= %u", num, den, kPvMaxDen); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

// (spsp_internal.h) the five checks every pass over sorted keys starts with, and what they establish about the arrays
int sorted_keys_front(spsp_ctx* ctx, const char* who_reads, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi,
                      const uint64_t* h_sk_off, uint32_t n, KeysShape* shape) {
    if (ctx->keys_unordered) { set_error("%s sorted sketches: not on a context switched to unordered keys", who_reads); return SPSP_ERR_ARG; }
    if (k < 1 || k > 63) { set_error("k=%u out of range 1..63", k); return SPSP_ERR_ARG; }
    for (uint32_t i = 0; i < n; ++i)
        if (h_sk_off[i + 1] < h_sk_off[i]) { set_error("sketch offsets must not decrease (sketch %u)", i); return SPSP_ERR_ARG; }
    const KeysShape s{k > 32, h_sk_off[0], h_sk_off[n], h_sk_off[n] - h_sk_off[0]};
    if (s.extent > 0xfffffff0ull) { set_error("too many sketch k-mers for one call"); return SPSP_ERR_OVERFLOW; }
    if (s.all_keys && (!d_mn || !d_lo || (s.has_hi && !d_hi))) { set_error("NULL key array"); return SPSP_ERR_ARG; }
    *shape = s;
    return SPSP_OK;
}

// (spsp_internal.h) the slots of a key table, as a power of two
uint32_t pv_table_log2cap(uint64_t entries) {
    const char* dbg_table = getenv("SPSP_DEBUG_PREVALENCE_TABLE");   // (read per call: a test switches it inside one process)
    const bool smallest = dbg_table && !strcmp(dbg_table, "min");
    const uint64_t want = std::max<uint64_t>(2, smallest ? entries : entries + entries / 2);
    uint32_t log2cap = 1;
    while (log2cap < kPvLog2CapMax && (1ull << log2cap) < want) ++log2cap;
    return log2cap;
}

// (spsp_internal.h) offsets, memset, k_pv_count, k_pv_read: what the prevalence pass and the selection both start with
int prevalence_fill_table(spsp_ctx* ctx, bool has_hi, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                          uint32_t n, uint32_t nq, bool claim, uint32_t* d_words) {
    int rc;
    ctx->cf_index.valid = false;                           // (a classification index is this table: it ends here)
    const uint64_t extent = h_sk_off[n], all_keys = h_sk_off[n] - h_sk_off[0], ref_keys = h_sk_off[n] - h_sk_off[nq];
    const uint32_t log2cap = ctx->pv_log2cap = pv_table_log2cap(ref_keys);   // (the table's size follows from the reference entries alone)
    const uint64_t cap = 1ull << log2cap;
    if ((rc = ctx->pv_off.reserve(((size_t)n + 1) * 8)) || (rc = ctx->pv_table.reserve((size_t)cap * 8)) ||
        (rc = ctx->pv_hold.reserve(std::max<size_t>(extent, 1) * 4))) return rc;
    uint64_t* d_off = ctx->pv_off.as<uint64_t>();
    unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
    uint32_t* d_hold = ctx->pv_hold.as<uint32_t>();
    const SortedKeys K{d_mn, d_lo, d_hi};
    SPSP_HIP(hipMemcpyAsync(d_off, h_sk_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (ref_keys) {
        SPSP_HIP(hipMemsetAsync(d_tbl, 0, (size_t)cap * 8, ctx->stream));
        const uint32_t gx = (uint32_t)((ref_keys + kPvThreads - 1) / kPvThreads);
        if (has_hi) hipLaunchKernelGGL(k_pv_count<true>, dim3(gx), dim3(kPvThreads), 0, ctx->stream, K, (const uint64_t*)d_off, n, nq, d_tbl, log2cap, d_words);
        else hipLaunchKernelGGL(k_pv_count<false>, dim3(gx), dim3(kPvThreads), 0, ctx->stream, K, (const uint64_t*)d_off, n, nq, d_tbl, log2cap, d_words);
    }
    if (all_keys) {
        if (!ref_keys) SPSP_HIP(hipMemsetAsync(d_tbl, 0, (size_t)cap * 8, ctx->stream));   // (queries against references without keys: all absent)
        const uint32_t gx = (uint32_t)((all_keys + kPvThreads - 1) / kPvThreads);
        auto read = has_hi ? (claim ? k_pv_read<true, true> : k_pv_read<true, false>) : (claim ? k_pv_read<false, true> : k_pv_read<false, false>);
        hipLaunchKernelGGL(read, dim3(gx), dim3(kPvThreads), 0, ctx->stream, K, (const uint64_t*)d_off, n, nq, (const unsigned long long*)d_tbl, log2cap, d_hold,
                           d_words);
    }
    SPSP_HIP(hipGetLastError());
    return SPSP_OK;
}

int prevalence_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off,
                           uint32_t n, uint32_t nq, uint32_t num, uint32_t den, spsp_prevalence_row* rows, uint64_t* spectrum, uint32_t** d_holders) {
    int rc;
    if (d_holders) *d_holders = nullptr;
    if ((rc = prevalence_check_args(n, nq, num, den))) return rc;
    KeysShape shape;
    if ((rc = sorted_keys_front(ctx, "prevalence reads", k, d_mn, d_lo, d_hi, h_sk_off, n, &shape))) return rc;
    const bool has_hi = shape.has_hi;
    const uint32_t R = n - nq, n_rows = nq ? nq : n;
    const uint64_t ref_keys = h_sk_off[n] - h_sk_off[nq];
    const uint32_t core_min = (uint32_t)(((uint64_t)num * R + den - 1) / den);       // h * den >= num * R  <=>  h >= ceil(num * R / den)
    const size_t spec_bytes = (size_t)kPvWords * 4 + ((size_t)R + 1) * 8;
    if ((rc = ctx->pv_rows.reserve((size_t)n_rows * sizeof(spsp_prevalence_row))) || (rc = ctx->pv_spec.reserve(spec_bytes))) return rc;
    spsp_prevalence_row* d_rows = ctx->pv_rows.as<spsp_prevalence_row>();
    uint32_t* d_words = ctx->pv_spec.as<uint32_t>();
    unsigned long long* d_spec = reinterpret_cast<unsigned long long*>(d_words + kPvWords);
    SPSP_HIP(hipMemsetAsync(d_words, 0, spec_bytes, ctx->stream));
    if ((rc = prevalence_fill_table(ctx, has_hi, d_mn, d_lo, d_hi, h_sk_off, n, nq, false, d_words))) return rc;
    const uint64_t* d_off = ctx->pv_off.as<uint64_t>();
    const unsigned long long* d_tbl = ctx->pv_table.as<unsigned long long>();
    uint32_t* d_hold = ctx->pv_hold.as<uint32_t>();
    const uint64_t cap = 1ull << ctx->pv_log2cap;
    hipLaunchKernelGGL(k_pv_rows, dim3(n_rows), dim3(kPvThreads), 0, ctx->stream, (const uint32_t*)d_hold, (const uint64_t*)d_off, core_min, d_rows);
    if (ref_keys) {
        const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((cap + kPvThreads - 1) / kPvThreads, (uint64_t)std::max(ctx->n_cu, 1) * kPvSpecBlocksPerCu));
        hipLaunchKernelGGL(k_pv_spectrum, dim3(gx, R / kPvWindow + 1), dim3(kPvThreads), 0, ctx->stream, (const unsigned long long*)d_tbl, cap, R, d_spec);
    }
    SPSP_HIP(hipGetLastError());
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsPvBad, d_words, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(rows, d_rows, (size_t)n_rows * sizeof(spsp_prevalence_row), hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(spectrum, d_spec, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait
    if (ctx->h_scalar[kHsPvBad]) {
        set_error("sketch keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)");
        memset(rows, 0, (size_t)n_rows * sizeof(spsp_prevalence_row));
        memset(spectrum, 0, ((size_t)R + 1) * 8);
        return SPSP_ERR_ARG;
    }
    if (d_holders) *d_holders = d_hold;
    return SPSP_OK;
}

// spsp_prevalence_files behind its argument checks: the sketches loaded (spsp_host.cpp), decoded (and brought down to the common
// rate), the prevalence pass, <out_prefix>_prevalence.csv.gz and <out_prefix>_spectrum.csv.gz
static int prevalence_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, uint32_t num, uint32_t den,
                            const char* out_prefix, int chatter, double rate, std::vector<spsp_prevalence_row>* rows, std::vector<uint64_t>* spectrum) {
    FilesRun run(ctx, paths, n, chatter);
    int rc = run.begin(run.refuse_k_eq_m(run.load(rate), "prevalence is"));   // (the k == m refusal in front of the rate's own)
    if (rc) return rc;
    const uint32_t R = n - n_query, n_rows = n_query ? n_query : n;
    rows->assign(n_rows, spsp_prevalence_row{});
    spectrum->assign((size_t)R + 1, 0);
    rc = run.decode();
    const DecodedKeys& keys = run.keys;
    if (!rc) rc = prevalence_device_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), n, n_query, num, den, rows->data(), spectrum->data(), nullptr);
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_prevalence_csv_host(rows->data(), n_rows, paths, run.card.data(), precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_prevalence.csv.gz", t1))) return rc;
    const double t2 = now_s();
    if ((rc = spsp_spectrum_csv_host(spectrum->data(), R, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_spectrum.csv.gz", t2)) || !chatter) return rc;
    const uint32_t core_min = (uint32_t)(((uint64_t)num * R + den - 1) / den);
    uint64_t in_union = 0, in_core = 0;
    for (uint32_t t = 1; t <= R; ++t) { in_union += (*spectrum)[t]; if (t >= core_min) in_core += (*spectrum)[t]; }
    printf("%u reference(s), %llu distinct keys, %llu of them core (held by %u references or more)\n", R, (unsigned long long)in_union,
           (unsigned long long)in_core, core_min);
    say_common_rate(run.L, n);
    fflush(stdout);
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_prevalence_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi,
                                      const uint64_t* h_sk_off, uint32_t n, uint32_t n_query, uint32_t num, uint32_t den, spsp_prevalence_row* rows,
                                      uint64_t* spectrum, void** d_holders) {
    if (d_holders) *d_holders = nullptr;
    if (!ctx || !h_sk_off || !rows || !spectrum) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint32_t* held = nullptr;
    const int rc = prevalence_device_impl(ctx, k, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n, n_query,
                                          num, den, rows, spectrum, &held);
    if (d_holders) *d_holders = held;
    return rc;
}

extern "C" int spsp_prevalence_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, uint32_t n_query, int precision, uint32_t num, uint32_t den,
                                     const char* out_prefix, int chatter, double rate, spsp_prevalence_row** rows, uint64_t** spectrum) {
    if (rows) *rows = nullptr;
    if (spectrum) *spectrum = nullptr;
    if (!ctx || !paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = prevalence_check_args(n, n_query, num, den))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_prevalence_row> got;
    std::vector<uint64_t> spec;
    if ((rc = prevalence_files(ctx, paths, n, n_query, precision, num, den, out_prefix, chatter, rate, &got, &spec))) return rc;
    if (rows && (rc = give_rows(got, rows))) return rc;
    if (spectrum && (rc = give_rows(spec, spectrum))) { if (rows) { free(*rows); *rows = nullptr; } return rc; }
    return SPSP_OK;
}
