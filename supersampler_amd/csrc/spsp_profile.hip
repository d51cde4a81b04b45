// Profile on the GPU: which references a read set holds, each shared key counted once, and how deep each one is (not in the
// reference).  The greedy rounds of gather (spsp_gather.hip) on the counters of the depth pass (spsp_depth.hip); the rule is in
// include/spsp.h.  Everything the rounds need is on the device behind the adds: the index's key-major holder lists (key_start,
// list), a key number per index entry (dp_kn), a counter per distinct key (dp_count), and a reduction that takes a class byte per
// entry.  The edges gather spends a match pass, two scans and a fill on are the index itself.
//
// start (once per call):
//   k_dp_entry   as a read: c_e[at] = count[kn[at]], and the word of the keys found = |F|.
//   k_pf_start   a workgroup per 2 048 index entries: u[reference of the entry] += (c_e >= min_count), one add per wave where the
//                tile's entries belong to one reference (two searches of the offsets per tile), else a short search and an add
//                per found entry; the entries below D add the found counts up to the 64-bit found_sum (one add per wave).  dead[D], assigned[E] and
//                the state words are cleared in front of it.  Bound: 4 bytes per entry.
// round (pick + walk, queued kPfBatchFirst, then twice as many, up to kPfBatchMax per host wait):
//   k_pf_pick    one workgroup of 1 024 lanes: arg-max over u[0 .. R) as (u << 32 | ~j) words, so the tie rule is a property of the
//                maximum; lane 0 stops the call or writes the round's (reference, assigned, remaining), names the winner and zeroes
//                its counter.  A stopped call's launches return at their first load.
//   k_pf_walk    waves over the WINNER'S entries, 16 at a time, dealt over the workgroups first (a reference of 6 000 keys is then on
//                a hundred CUs and more).  Entry e with c_e >= min_count and dead[kn[e]] == 0: dead = 1, assigned[e] = 1 (plain stores:
//                a reference's keys are distinct, so exactly one lane of one round touches a key), and every OTHER holder in the
//                key's list gets one no-return atomicSub on its u.  A list of more than kPfListCut holders is walked by the whole
//                wave: 64 consecutive 16-bit holder numbers per load, and where the list is ascending 64 neighbouring counters
//                per atomic instruction.  A key that is alive is held by no earlier winner (that winner took it), so no counter
//                goes below zero.  Up to kCfLdsRefs references the decrements are LDS atomics on a counter per reference and
//                workgroup, taken off u once behind the workgroup's walk (the keys of one winner are held by the same few
//                references: a device atomic per holder queues on their counters); beyond, the plain form.
// statistics: ONE run of the depth reduction (depth_launch_reduce) with assigned[] in the place of the unique bytes: its five
//   unique_ outputs are the assigned five, exact lower median, radix select and long references included.
// No workgroup waits for another: the order of rounds is the order of launches on the stream.  Host waits: one per batch, one
// for the statistics.
#include <algorithm>
#include <cstring>
#include <vector>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kNoWinner = 0xffffffffu;
constexpr uint32_t kPfWaveEntries = 16;                   // k_pf_walk: the winner's entries one wave takes at a time
// the words the round kernels keep (cleared per call; copied out once per batch)
struct PfState { uint32_t alive, stopped, n_rows, winner; unsigned long long found_sum, pad; };
// one round as k_pf_pick leaves it
struct PfRound { uint32_t reference, assigned, remaining, pad; };

// off: the references' first entries (absolute; off[0] = the index's first entry); c_e: c per index entry; count: c per distinct key.
// A workgroup takes kPfStartTile consecutive entries: two searches of the offsets for the tile's ends, and every other search
// between their answers (measured with a search pair per 256 entries: the searches, not the stream, were the kernel's time)
constexpr uint32_t kPfStartTile = 2048, kPfStartPer = kPfStartTile / kPfThreads;
constexpr uint32_t kPfStartSpan = 256;                     // a tile over at most this many references counts them in LDS
__global__ __launch_bounds__(kPfThreads) void k_pf_start(const uint64_t* __restrict__ off, uint32_t n_ref, uint32_t n_index, const uint32_t* __restrict__ c_e,
                                                         const uint32_t* __restrict__ count, uint32_t D, uint32_t min_count, uint32_t* __restrict__ u,
                                                         PfState* __restrict__ state) {
    __shared__ uint32_t s_j[2];
    __shared__ uint32_t s_n[kPfStartSpan];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPfStartTile, i1 = min(i0 + kPfStartTile, (uint64_t)n_index), first = off[0];
    uint32_t c[kPfStartPer];                               // (the loads are on their way while lane 0 searches; 0 is below every min_count)
    unsigned long long v = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPfStartPer; ++q) { const uint64_t i = i0 + q * kPfThreads + threadIdx.x; c[q] = i < i1 ? c_e[i] : 0u; }
    // the sum of the found counts: the entries below D stand for the distinct keys (D <= n_index)
#pragma unroll
    for (uint32_t q = 0; q < kPfStartPer; ++q) {
        const uint64_t i = i0 + q * kPfThreads + threadIdx.x;
        if (i < D) { const uint32_t x = count[i]; if (x >= min_count) v += x; }
    }
    if (threadIdx.x == 0u) {                               // (i0 < n_index: the grid is the entries' size)
        s_j[0] = sorted_sketch_of(off, 0, n_ref, first + i0);
        s_j[1] = sorted_sketch_of(off, 0, n_ref, first + i1 - 1u);
    }
    s_n[threadIdx.x] = 0u;                                 // (kPfStartSpan == kPfThreads)
    __syncthreads();
    const uint32_t j0 = s_j[0], j1 = s_j[1];
    const bool one = j0 == j1, few = j1 - j0 < kPfStartSpan;   // (uniform)
    uint32_t n = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPfStartPer; ++q) {
        if (c[q] < min_count) continue;
        if (one) { ++n; continue; }                        // one reference: counted in registers, an add per wave
        const uint32_t j = sorted_sketch_of(off, j0, j1 + 1u, first + i0 + q * kPfThreads + threadIdx.x);
        if (few) atomicAdd(&s_n[j - j0], 1u); else atomicAdd(&u[j], 1u);
    }
    n = wave_sum(n); v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0u) {
        if (n) atomicAdd(&u[j0], n);
        if (v) atomicAdd(&state->found_sum, v);
    }
    if (!one && few) {
        __syncthreads();
        const uint32_t m = s_n[threadIdx.x];
        if (m) atomicAdd(&u[j0 + threadIdx.x], m);         // (m != 0 only below the span: j0 + lane <= j1)
    }
}
static_assert(kPfStartSpan == kPfThreads, "a lane clears and flushes one LDS counter");

// found: the 64-bit word of the keys found (|F|), which the first round starts from; slot: this launch's place in the batch's records
__global__ __launch_bounds__(kPfPickThreads) void k_pf_pick(uint32_t* __restrict__ u, uint32_t n_ref, uint32_t min_keys, uint32_t max_rounds,
                                                            PfState* __restrict__ state, const unsigned long long* __restrict__ found,
                                                            PfRound* __restrict__ rounds, uint32_t slot) {
    __shared__ unsigned long long s_best[kPfPickThreads];
    const uint32_t t = threadIdx.x;
    if (state->stopped) return;                            // (uniform: every lane reads the same word)
    unsigned long long best = 0;                           // value first, then the LOWEST index: u << 32 | ~j
    for (uint32_t j = t; j < n_ref; j += kPfPickThreads) {
        const unsigned long long w = (unsigned long long)u[j] << 32 | (0xffffffffu - j);
        best = w > best ? w : best;
    }
    s_best[t] = best;
    __syncthreads();
#pragma unroll
    for (uint32_t d = kPfPickThreads / 2; d; d >>= 1) {
        if (t < d) { const unsigned long long o = s_best[t + d]; if (o > s_best[t]) s_best[t] = o; }
        __syncthreads();
    }
    if (t != 0) return;
    const unsigned long long top = s_best[0];
    const uint32_t best_u = (uint32_t)(top >> 32), j = 0xffffffffu - (uint32_t)top, rank = state->n_rows + 1u;
    if (best_u < min_keys || j >= n_ref || (max_rounds && rank > max_rounds)) {   // (j >= n_ref: no reference at all, best is 0)
        state->stopped = 1u;
        state->winner = kNoWinner;
        return;
    }
    const uint32_t left = (rank == 1u ? (uint32_t)*found : state->alive) - best_u;
    PfRound r;
    r.reference = j; r.assigned = best_u; r.remaining = left; r.pad = 0;
    rounds[slot] = r;
    state->alive = left;
    state->n_rows = rank;
    state->winner = j;
    u[j] = 0;                                              // all its live keys die in this round: it is never named again
}

// kn, c_e, assigned: per index entry; dead: per distinct key; key_start [D + 1], list: the index's key-major form.  LDS: the workgroup
// counts what it takes off every reference in n_ref words of LDS and takes it off u once, behind its walk
template <bool LDS>
__global__ __launch_bounds__(kPfThreads) void k_pf_walk(const uint64_t* __restrict__ off, const uint32_t* __restrict__ kn, const uint32_t* __restrict__ c_e,
                                                        const uint32_t* __restrict__ key_start, const uint16_t* __restrict__ list, uint32_t D, uint32_t min_count,
                                                        uint32_t n_ref, uint32_t* __restrict__ u, uint8_t* __restrict__ dead, uint8_t* __restrict__ assigned,
                                                        const PfState* __restrict__ state) {
    extern __shared__ uint32_t s_off[];                    // (LDS form: n_ref words)
    const uint32_t j = state->winner;
    if (j == kNoWinner) return;                            // (uniform)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = off[0], a = off[j] - first, z = off[j + 1] - first;
    // waves take kPfWaveEntries entries at a time (the first lanes; every lane walks the long lists: measured with 64 entries per
    // wave, a species' first rounds sat on a hundred waves that each walked a dozen lists of thousands of holders one after the
    // other), wave w of workgroup b being wave w * gridDim.x + b: the workgroups fill before their waves do
    if (a + (uint64_t)blockIdx.x * kPfWaveEntries >= z) return;   // (uniform: its first wave has nothing, so none has)
    if (LDS) {
        for (uint32_t r = threadIdx.x; r < n_ref; r += kPfThreads) s_off[r] = 0u;
        __syncthreads();
    }
    auto take_off = [&](uint32_t o) {                      // (the value is not used: an atomic without a return)
        if (o == j) return;
        if (LDS) atomicAdd(&s_off[o], 1u); else atomicSub(&u[o], 1u);
    };
    const uint64_t mine = (uint64_t)(threadIdx.x >> 6) * gridDim.x + blockIdx.x, waves = (uint64_t)gridDim.x * (kPfThreads / 64u);
    for (uint64_t base = a + mine * kPfWaveEntries; base < z; base += waves * kPfWaveEntries) {   // (uniform per wave)
        const uint64_t i = base + lane;
        bool take = false;
        uint32_t ls = 0, len = 0;
        if (lane < kPfWaveEntries && i < z && c_e[i] >= min_count) {
            const uint32_t d = kn[i];
            if (d < D && !dead[d]) {                       // (the winner's keys are distinct: no other lane holds this one)
                take = true;
                dead[d] = 1;
                assigned[i] = 1;
                ls = key_start[d];
                len = key_start[d + 1u] - ls;
            }
        }
        if (take && len <= kPfListCut)
            for (uint32_t h = 0; h < len; ++h) take_off(list[ls + h]);
        unsigned long long left = __ballot(take && len > kPfListCut);
        while (left) {                                     // the long lists, one after another by the whole wave (wave_long_lists moved its registers: DESIGN 6v)
            const int l = __ffsll((long long)left) - 1;
            const uint32_t s0 = __shfl(ls, l), n0 = __shfl(len, l);
            for (uint32_t h = lane; h < n0; h += 512u) {   // eight loads in flight in front of their eight adds
                uint32_t o[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) o[q] = h + 64u * q < n0 ? list[s0 + h + 64u * q] : j;
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) take_off(o[q]);
            }
            left &= left - 1ull;
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t r = threadIdx.x; r < n_ref; r += kPfThreads) { const uint32_t v = s_off[r]; if (v) atomicSub(&u[r], v); }
    }
}

const char* const kNoCounters = "profile: the context holds no counters (spsp_depth_begin_device first; they end with the index they were made for)";

int check_args(uint32_t min_count, uint32_t min_keys) {
    if (min_count == 0) { set_error("profile: min_count is at least 1 (a key no record holds is not found)"); return SPSP_ERR_ARG; }
    if (min_keys == 0) { set_error("profile: min_keys is at least 1 (a reference without a live key is never named)"); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

}  // namespace

int profile_impl(spsp_ctx* ctx, uint32_t min_count, uint32_t min_keys, uint32_t max_rounds, spsp_profile_row* rows, uint64_t* n_rows, spsp_profile_totals* totals,
                 const uint8_t** d_entry_assigned) {
    int rc;
    const spsp_ctx::ClassifyIndex& X = ctx->cf_index;
    *n_rows = 0;
    if (d_entry_assigned) *d_entry_assigned = nullptr;
    if (totals) memset(totals, 0, sizeof *totals);
    if (!X.valid || !X.depth) { set_error("%s", kNoCounters); return SPSP_ERR_ARG; }
    if ((rc = check_args(min_count, min_keys))) return rc;
    const uint32_t R = X.n_ref, E = X.entries, D = X.distinct;
    ctx->pf_last[0] = ctx->pf_last[1] = ctx->pf_last[2] = 0;
    if ((rc = ctx->pf_u.reserve((size_t)R * 4)) || (rc = ctx->pf_dead.reserve((size_t)D + 64)) || (rc = ctx->pf_assigned.reserve((size_t)E + 64)) ||
        (rc = ctx->pf_state.reserve(sizeof(PfState))) || (rc = ctx->pf_rounds.reserve(kPfBatchMax * sizeof(PfRound))) ||
        (rc = ctx->pf_rows.reserve((size_t)R * sizeof(spsp_depth_row)))) return rc;
    if (d_entry_assigned) *d_entry_assigned = ctx->pf_assigned.as<uint8_t>();
    if (E == 0) return SPSP_OK;                            // (an index without a key: nothing is found)
    uint32_t* d_u = ctx->pf_u.as<uint32_t>();
    uint8_t *d_dead = ctx->pf_dead.as<uint8_t>(), *d_assigned = ctx->pf_assigned.as<uint8_t>();
    PfState* d_state = ctx->pf_state.as<PfState>();
    PfRound* d_rounds = ctx->pf_rounds.as<PfRound>();
    const uint64_t* d_off = ctx->pv_off.as<uint64_t>();
    const uint32_t* d_c = nullptr;
    hipEvent_t* ev = nullptr;                              // [0], [1] around the start, [2], [3] around the reduction, [4 ...] a batch's picks and walks
    if (ctx->timing) {
        ctx->pf_events.resize(4 + 2 * kPfBatchMax + 1, nullptr);
        for (hipEvent_t& e : ctx->pf_events) if (!e) SPSP_HIP(hipEventCreate(&e));
        ev = ctx->pf_events.data();
    }
    if (ev) SPSP_HIP(hipEventRecord(ev[0], ctx->stream));
    unsigned long long* d_found = nullptr;
    if ((rc = depth_launch_entry(ctx, min_count, &d_found))) return rc;
    d_c = ctx->dp_entry.as<uint32_t>();
    SPSP_HIP(hipMemsetAsync(d_u, 0, (size_t)R * 4, ctx->stream));
    SPSP_HIP(hipMemsetAsync(d_dead, 0, (size_t)D, ctx->stream));
    SPSP_HIP(hipMemsetAsync(d_assigned, 0, (size_t)E, ctx->stream));
    SPSP_HIP(hipMemsetAsync(d_state, 0, sizeof(PfState), ctx->stream));
    hipLaunchKernelGGL(k_pf_start, dim3((uint32_t)(((uint64_t)E + kPfStartTile - 1) / kPfStartTile)), dim3(kPfThreads), 0, ctx->stream, d_off, R, E, d_c,
                       (const uint32_t*)ctx->dp_count.as<uint32_t>(), D, min_count, d_u, d_state);
    SPSP_HIP(hipGetLastError());
    if (ev) SPSP_HIP(hipEventRecord(ev[1], ctx->stream));
    uint64_t max_ref = 0;
    for (uint32_t j = 0; j < R; ++j) max_ref = std::max(max_ref, X.off_host[j + 1] - X.off_host[j]);
    // up to kCfLdsRefs references a workgroup's decrements go through LDS (measured: the plain form spends a round on the same few
    // counters -- a family's, a species' -- one atomic after the other); then all four waves of a workgroup get entries
    const bool in_lds = R <= kCfLdsRefs;
    const size_t walk_lds = in_lds ? (size_t)R * 4 : 0;
    const uint64_t chunks = (max_ref + kPfWaveEntries - 1u) / kPfWaveEntries, cus = (uint64_t)std::max(ctx->n_cu, 1);
    const uint32_t walk_blocks = (uint32_t)std::max<uint64_t>(1, in_lds ? std::min(cus, (chunks + 3u) / 4u) : std::min(cus * 2u, chunks));
    if (in_lds && (rc = lds_opt_in(ctx, &k_pf_walk<true>, kAcLdsBytes))) return rc;
    std::vector<PfRound> named;
    PfRound got[kPfBatchMax];
    PfState st{};
    unsigned long long found_keys = 0;
    uint32_t done = 0, batch = kPfBatchFirst, waits = 0;
    for (;;) {
        uint32_t B = batch;
        if (max_rounds) B = std::min(B, max_rounds - done);
        for (uint32_t s = 0; s < B; ++s) {
            if (ev) SPSP_HIP(hipEventRecord(ev[4 + 2 * s], ctx->stream));
            hipLaunchKernelGGL(k_pf_pick, dim3(1), dim3(kPfPickThreads), 0, ctx->stream, d_u, R, min_keys, max_rounds, d_state, (const unsigned long long*)d_found,
                               d_rounds, s);
            if (ev) SPSP_HIP(hipEventRecord(ev[4 + 2 * s + 1], ctx->stream));
            hipLaunchKernelGGL(in_lds ? &k_pf_walk<true> : &k_pf_walk<false>, dim3(walk_blocks), dim3(kPfThreads), walk_lds, ctx->stream, d_off,
                               (const uint32_t*)ctx->dp_kn.as<uint32_t>(), d_c, X.key_start, X.list, D, min_count, R, d_u, d_dead, d_assigned, (const PfState*)d_state);
        }
        SPSP_HIP(hipGetLastError());
        if (ev) SPSP_HIP(hipEventRecord(ev[4 + 2 * B], ctx->stream));
        SPSP_HIP(hipMemcpyAsync(got, d_rounds, (size_t)B * sizeof(PfRound), hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipMemcpyAsync(&st, d_state, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipMemcpyAsync(&found_keys, d_found, 8, hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // one wait per batch of rounds
        ++waits;
        if (ev) {
            if (done == 0) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); ctx->pf_ms[0] += ms; }
            for (uint32_t s = 0; s < 2 * B; ++s) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ev[4 + s], ev[4 + s + 1])); ctx->pf_ms[1 + (s & 1u)] += ms; }
        }
        done += B;
        // the rounds of this batch sit in its first slots: every launch names one until the call stops, then none does
        const uint32_t fresh = st.n_rows - (uint32_t)named.size();
        if (st.n_rows > R || fresh > B) { set_error("profile: %u rounds for %u references (the index arrays changed during the call?)", st.n_rows, R); return SPSP_ERR_ARG; }
        named.insert(named.end(), got, got + fresh);
        if (st.stopped || named.size() == R || (max_rounds && done >= max_rounds)) break;
        batch = std::min(kPfBatchMax, batch * 2);
    }
    ctx->pf_last[0] = done; ctx->pf_last[1] = (uint32_t)named.size();
    if (totals) { totals->found_keys = (uint32_t)found_keys; totals->found_sum = st.found_sum; }
    if (!named.empty()) {
        std::vector<spsp_depth_row> reduced(R);
        if (ev) SPSP_HIP(hipEventRecord(ev[2], ctx->stream));
        if ((rc = depth_launch_reduce(ctx, d_assigned, min_count, ctx->pf_rows.as<spsp_depth_row>()))) return rc;
        if (ev) SPSP_HIP(hipEventRecord(ev[3], ctx->stream));
        SPSP_HIP(hipMemcpyAsync(reduced.data(), ctx->pf_rows.p, (size_t)R * sizeof(spsp_depth_row), hipMemcpyDeviceToHost, ctx->stream));
        SPSP_HIP(hipStreamSynchronize(ctx->stream));       // the wait for the statistics
        ++waits;
        if (ev) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ev[2], ev[3])); ctx->pf_ms[3] += ms; }
        for (size_t r = 0; r < named.size(); ++r) {
            const spsp_depth_row& d = reduced[named[r].reference];
            if (d.unique_found != named[r].assigned) {
                set_error("profile: round %zu assigned %u key(s) of reference %u, its reduction counts %u (the counters changed during the call?)", r + 1,
                          named[r].assigned, named[r].reference, d.unique_found);
                return SPSP_ERR_ARG;
            }
            spsp_profile_row& row = rows[r];
            row.sum = d.unique_sum; row.reference = named[r].reference; row.keys = d.keys; row.found = d.found; row.assigned = named[r].assigned;
            row.median = d.unique_median; row.max = d.unique_max; row.remaining = named[r].remaining; row.reserved = 0;
            if (totals) { totals->assigned_keys += row.assigned; totals->assigned_sum += row.sum; }
        }
    }
    ctx->pf_last[2] = waits;
    *n_rows = named.size();
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_profile_device(spsp_ctx* ctx, uint32_t min_count, uint32_t min_keys, uint32_t max_rounds, spsp_profile_row* rows, uint64_t* n_rows,
                                   spsp_profile_totals* totals, const void** d_entry_assigned) {
    if (d_entry_assigned) *d_entry_assigned = nullptr;
    if (n_rows) *n_rows = 0;
    if (!ctx || !rows || !n_rows) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    const uint8_t* d = nullptr;
    const int rc = profile_impl(ctx, min_count, min_keys, max_rounds, rows, n_rows, totals, &d);
    if (d_entry_assigned) *d_entry_assigned = rc == SPSP_OK ? d : nullptr;
    return rc;
}

extern "C" int spsp_profile_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (int i = 0; i < 4; ++i) { ms[i] = ctx->pf_ms[i]; ctx->pf_ms[i] = 0; }
    return SPSP_OK;
}

extern "C" int spsp_profile_counts(spsp_ctx* ctx, uint32_t* counts) {
    if (!ctx || !counts) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (int i = 0; i < 3; ++i) counts[i] = ctx->pf_last[i];
    return SPSP_OK;
}

extern "C" int spsp_profile_files(spsp_ctx* ctx, const char* const* index_paths, uint32_t n_ref, const char* const* reads_paths, uint32_t n_reads, uint32_t min_count,
                                  uint32_t min_keys, uint32_t max_rounds, int precision, const char* out_prefix, int chatter, double rate, spsp_depth_row** rows,
                                  spsp_depth_totals* totals, spsp_profile_row** profile_rows, uint64_t* n_profile_rows, spsp_profile_totals* profile_totals) {
    if (rows) *rows = nullptr;
    if (profile_rows) *profile_rows = nullptr;
    if (n_profile_rows) *n_profile_rows = 0;
    spsp_depth_totals mine{};
    if (totals) *totals = mine;
    if (profile_totals) memset(profile_totals, 0, sizeof *profile_totals);
    if (!ctx || !index_paths || !reads_paths || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (uint32_t f = 0; f < n_reads; ++f) if (!reads_paths[f]) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n_ref == 0 || n_ref > 65535) { set_error("a classification index takes 1 .. 65535 references (n = %u)", n_ref); return SPSP_ERR_ARG; }
    if (n_reads == 0) { set_error("profile takes at least one reads file"); return SPSP_ERR_ARG; }
    int rc;
    if ((rc = check_args(min_count, min_keys))) return rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_depth_row> got;
    ProfileAsk ask{};
    ask.min_keys = min_keys; ask.max_rounds = max_rounds;
    if ((rc = depth_files_impl(ctx, index_paths, n_ref, reads_paths, n_reads, min_count, precision, out_prefix, chatter, rate, &got, &mine, &ask))) return rc;
    if (totals) *totals = mine;
    if (profile_totals) *profile_totals = ask.totals;
    if (n_profile_rows) *n_profile_rows = ask.rows.size();
    if (rows && (rc = give_rows(got, rows))) return rc;
    if (profile_rows && (rc = give_rows(ask.rows, profile_rows))) return rc;
    return SPSP_OK;
}
