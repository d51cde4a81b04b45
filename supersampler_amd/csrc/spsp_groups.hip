// Groups on the GPU: per group of a partitioned collection the keys it holds, shares, holds alone, and is identified by (not in
// the reference, whose end product is the two n x n matrices).
//
// Keys and notation are the prevalence pass's (spsp_prevalence.hip): sketches 0 .. n-1 back to back, each sorted by (minimizer,
// kmer_hi, kmer_lo); every sketch takes part.  group[i] in 0 .. G-1; h(x) = the sketches that hold key x, h_c(x) = the members of
// group c that hold it.  For group c a key is present (h_c >= 1), core (h_c >= in_min_c), exclusive (h_c == h) and a marker (core
// and h - h_c <= out_max_c); in_min and out_max come from spsp_groups_bounds_host.  Integers only.
//
// One chain of launches whatever the sketches are:
//   table fill    prevalence's own (prevalence_fill_table, all versus all): pv_hold[e] = h of entry e, with the order check
//   k_gp_count    a lane per entry: its CELL's slot in a second table -- the first free slot of the probe sequence from a home hashed
//                 from the key AND the entry's group, claimed by one CAS of (entry + 1 | group << 32), or the slot whose word names
//                 the same group and whose claimer holds the same full key -- and one atomic add on the word's top 16 bits.  A
//                 counter ends at size_c <= 65 535: it cannot carry out.  The group of a probed slot sits in the word: no probe
//                 searches the offsets
//   k_gp_read     a lane per entry: the same probe sequence without the claim.  The lane has h, h_c and its group's two bounds in
//                 registers, so the key's four properties are decided HERE, once: cell[e] = h_c | core << 28 | exclusive << 29 |
//                 marker << 30 | (e claimed the cell) << 31.  One occurrence per (key, group) carries bit 31
//   k_gp_rows     a workgroup per sketch over its slice of cell[]: the member row over all its entries, the four group counters
//                 over its claiming entries; lane 0 writes one record per sketch, no global atomic.  The host adds the records of
//                 a group's members: which member claimed a cell is a race, the sum over the group is not
//   markers only  ds_flag_compact_launch (k_ds_flag_band: claimers whose cell is a marker -> k_ds_flag's keep mask; the compaction with
//                 the sketch bounds: every sketch's surviving run), k_gp_regroup (a workgroup per sketch moves its run to its group's region: the
//                 members' runs in list order), big_sort_segments over the regions made of more than one run
// Host waits: one (records, flag words, and with markers the compacted offsets); with markers the sort's own behind it.  No wait
// depends on the data beyond sizing the output and the sort, and no workgroup ever waits for another one.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

constexpr uint32_t kGpThreads = 256;                       // 4 waves, every kernel
enum { kGpwBad = 0, kGpwWrapped = 1, kGpwCell = 2, kGpWords = 4 };   // flag words: the first fill's two, the cell table's, one spare
constexpr uint32_t kGpCore = 1u << 28, kGpExclusive = 1u << 29, kGpMarker = 1u << 30, kGpClaim = 1u << 31;   // cell[e]: h_c below them
constexpr uint32_t kGpRecord = 7;                          // u64 per sketch: member core, exclusive, marker | claimed present, core, exclusive, marker

struct GpBound { uint32_t in_min, out_max; };

// a cell's home: pv_home's hash of the key (left as it is), mixed with the group
template <bool HAS_HI>
__device__ __forceinline__ uint64_t gp_home(uint32_t mn, uint64_t hi, uint64_t lo, uint32_t g, uint32_t log2cap) {
    uint64_t h = xxh64_u64(lo + (uint64_t)(mn + 1u) * 0x9E3779B97F4A7C15ULL);
    if (HAS_HI) h = xxh64_u64(h ^ hi);
    h = xxh64_u64(h ^ ((uint64_t)(g + 1u) * 0xC2B2AE3D27D4EB4FULL));
    return h >> (64u - log2cap);                           // (log2cap >= 1)
}

// a slot word: the claimer's entry number + 1 in bits 0..31 (0: free), the group in bits 32..47, the members counted so far above
__device__ __forceinline__ bool gp_names(unsigned long long word, uint32_t g) { return (uint32_t)(word >> 32 & 0xffffull) == g; }

template <bool HAS_HI>
__global__ __launch_bounds__(kGpThreads) void k_gp_count(SortedKeys K, const uint64_t* __restrict__ off, uint32_t n, const uint16_t* __restrict__ grp,
                                                         unsigned long long* __restrict__ tbl, uint32_t log2cap, uint32_t* __restrict__ words) {
    const uint64_t e = off[0] + (uint64_t)blockIdx.x * kGpThreads + threadIdx.x;
    if (e >= off[n]) return;
    const uint32_t g = grp[sorted_sketch_of(off, 0, n, e)];
    const uint32_t mn = K.mn[e];
    const uint64_t lo = K.lo[e], hi = HAS_HI ? K.hi[e] : 0ull;
    const uint64_t mask = (1ull << log2cap) - 1ull;
    const unsigned long long mine = (unsigned long long)((uint32_t)e + 1u) | (unsigned long long)g << 32;
    uint64_t pos = gp_home<HAS_HI>(mn, hi, lo, g, log2cap);
    for (uint64_t probes = 0;; ++probes) {
        // (a stale 0 only costs the CAS, which answers with the word as it is; a word's low 48 bits never change once claimed)
        unsigned long long cur = tbl[pos];
        if ((uint32_t)cur == 0u) cur = atomicCAS(&tbl[pos], 0ull, mine);
        if ((uint32_t)cur == 0u) break;                    // claimed
        if (gp_names(cur, g) && pv_same<HAS_HI>(K, (uint64_t)((uint32_t)cur - 1u), mn, hi, lo)) break;
        // (never: the table has a slot per entry at the least and an entry claims one slot at the most)
        if (probes >= mask) { atomicOr(words + kGpwCell, 1u); return; }
        pos = (pos + 1ull) & mask;
    }
    atomicAdd(&tbl[pos], 1ull << 48);
}

template <bool HAS_HI>
__global__ __launch_bounds__(kGpThreads) void k_gp_read(SortedKeys K, const uint64_t* __restrict__ off, uint32_t n, const uint16_t* __restrict__ grp,
                                                        const GpBound* __restrict__ bound, const uint32_t* __restrict__ holders,
                                                        const unsigned long long* __restrict__ tbl, uint32_t log2cap, uint32_t* __restrict__ cell,
                                                        uint32_t* __restrict__ words) {
    const uint64_t e = off[0] + (uint64_t)blockIdx.x * kGpThreads + threadIdx.x;
    if (e >= off[n]) return;
    const uint32_t g = grp[sorted_sketch_of(off, 0, n, e)];
    const uint32_t mn = K.mn[e];
    const uint64_t lo = K.lo[e], hi = HAS_HI ? K.hi[e] : 0ull;
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t pos = gp_home<HAS_HI>(mn, hi, lo, g, log2cap);
    uint32_t v = 0;
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        const unsigned long long cur = tbl[pos];
        if ((uint32_t)cur == 0u) break;                    // (never: every entry went in)
        if (gp_names(cur, g) && pv_same<HAS_HI>(K, (uint64_t)((uint32_t)cur - 1u), mn, hi, lo)) {
            const uint32_t hc = (uint32_t)(cur >> 48), h = holders[e] & 0x7fffffffu;
            const GpBound b = bound[g];
            const uint32_t outside = h >= hc ? h - hc : 0xffffffffu;
            v = hc;
            if (hc >= b.in_min) v |= kGpCore;
            if (outside == 0u) v |= kGpExclusive;
            if (hc >= b.in_min && outside <= b.out_max) v |= kGpMarker;
            if ((uint32_t)cur - 1u == (uint32_t)e) v |= kGpClaim;
            break;
        }
        pos = (pos + 1ull) & mask;
    }
    if (v == 0u) atomicOr(words + kGpwCell, 1u);           // an entry without its cell
    cell[e] = v;
}

// one workgroup per sketch: record[i] = member core, exclusive, marker over all its entries | present, core, exclusive, marker over
// the entries that claimed their cell
__global__ __launch_bounds__(kGpThreads) void k_gp_rows(const uint32_t* __restrict__ cell, const uint64_t* __restrict__ off,
                                                        unsigned long long* __restrict__ record) {
    __shared__ unsigned long long s_part[kGpThreads / 64][kGpRecord];
    const uint32_t i = blockIdx.x, t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    const uint64_t end = off[i + 1];
    uint32_t c[kGpRecord] = {0, 0, 0, 0, 0, 0, 0};         // (per lane: fewer than 2^32 entries in all)
    for (uint64_t e = off[i] + t; e < end; e += kGpThreads) {
        const uint32_t v = cell[e];
        const uint32_t core = v >> 28 & 1u, excl = v >> 29 & 1u, mark = v >> 30 & 1u, claim = v >> 31;
        c[0] += core; c[1] += excl; c[2] += mark;
        c[3] += claim; c[4] += claim & core; c[5] += claim & excl; c[6] += claim & mark;
    }
#pragma unroll
    for (uint32_t f = 0; f < kGpRecord; ++f) {
        unsigned long long x = c[f];
#pragma unroll
        for (int d = 32; d; d >>= 1) x += __shfl_down(x, d);
        if (lane == 0) s_part[wid][f] = x;
    }
    __syncthreads();
    if (t >= kGpRecord) return;
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t w = 0; w < kGpThreads / 64; ++w) s += s_part[w][t];
    record[(size_t)i * kGpRecord + t] = s;
}

// one workgroup per sketch: its surviving run [run[i], run[i + 1]) of the compacted keys goes to dest[i] .. of the output
template <bool HAS_HI>
__global__ __launch_bounds__(kGpThreads) void k_gp_regroup(const uint32_t* __restrict__ mn, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi,
                                                           const uint64_t* __restrict__ run, const uint32_t* __restrict__ dest, uint32_t total,
                                                           uint32_t* __restrict__ out_mn, uint64_t* __restrict__ out_lo, uint64_t* __restrict__ out_hi) {
    const uint32_t i = blockIdx.x;
    const uint64_t a = run[i], z = run[i + 1];
    const uint64_t d = dest[i];
    if (z > total || z < a || d + (z - a) > total) return;  // (never: the host made dest from these very offsets)
    for (uint64_t j = threadIdx.x; j < z - a; j += kGpThreads) {
        out_mn[d + j] = mn[a + j];
        out_lo[d + j] = lo[a + j];
        if (HAS_HI) out_hi[d + j] = hi[a + j];
    }
}

void zero_results(spsp_group_row* rows, uint32_t n_groups, spsp_group_member_row* members, uint32_t n, uint64_t* marker_off) {
    if (rows && n_groups) memset(rows, 0, (size_t)n_groups * sizeof(spsp_group_row));
    if (members && n) memset(members, 0, (size_t)n * sizeof(spsp_group_member_row));
    if (marker_off) memset(marker_off, 0, ((size_t)n_groups + 1) * 8);
}

size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

}  // namespace

int groups_device_impl(spsp_ctx* ctx, uint32_t k, const uint32_t* d_mn, const uint64_t* d_lo, const uint64_t* d_hi, const uint64_t* h_sk_off, uint32_t n,
                       const uint32_t* h_group, uint32_t n_groups, uint32_t num, uint32_t den, uint32_t onum, uint32_t oden, spsp_group_row* rows,
                       spsp_group_member_row* members, bool want_markers, uint32_t** out_mn, uint64_t** out_lo, uint64_t** out_hi, uint64_t* marker_off) {
    int rc;
    *out_mn = nullptr; *out_lo = nullptr; *out_hi = nullptr;
    // (the sizes of what is zeroed must be sane before anything is: a refused n or n_groups zeroes nothing it cannot trust)
    const bool sized = n >= 1 && n <= 65535 && n_groups >= 1 && n_groups <= n;
    if (sized) zero_results(rows, n_groups, members, n, marker_off);
    std::vector<uint32_t> size(sized ? n_groups : 0), in_min(size.size()), out_max(size.size());
    if ((rc = spsp_groups_bounds_host(h_group, n, n_groups, num, den, onum, oden, size.data(), in_min.data(), out_max.data()))) return rc;
    KeysShape shape;
    if ((rc = sorted_keys_front(ctx, "groups read", k, d_mn, d_lo, d_hi, h_sk_off, n, &shape))) return rc;
    const bool has_hi = shape.has_hi;
    const uint64_t first = shape.first, extent = shape.extent, all_keys = shape.all_keys;
    for (uint32_t c = 0; c < n_groups; ++c) rows[c].members = size[c];
    for (uint32_t i = 0; i < n; ++i) rows[h_group[i]].entries += h_sk_off[i + 1] - h_sk_off[i];
    if (want_markers) {
        // (something to point at even when no key is a marker)
        if ((rc = ctx->gp_mn.reserve(64)) || (rc = ctx->gp_lo.reserve(64)) || (has_hi && (rc = ctx->gp_hi.reserve(64)))) return rc;
        *out_mn = ctx->gp_mn.as<uint32_t>(); *out_lo = ctx->gp_lo.as<uint64_t>(); *out_hi = has_hi ? ctx->gp_hi.as<uint64_t>() : nullptr;
    }
    if (all_keys == 0) return SPSP_OK;

    // the cell table: sized as the prevalence pass sizes its own -- the distinct (key, group) cells are never more than the entries
    const uint32_t log2cap = pv_table_log2cap(all_keys);
    const uint64_t cap = 1ull << log2cap;
    const uint32_t n_tiles = want_markers ? (uint32_t)((all_keys + kDsTile - 1) / kDsTile) : 0u, n_bounds = n + 1;
    // work area: flag words | the sketches' groups (16 bits each) | the groups' bounds | records | destinations | the compaction's part
    const size_t words_bytes = 64, grp_bytes = up64((size_t)n * 2), bound_bytes = up64((size_t)n_groups * sizeof(GpBound)),
                 rec_bytes = up64((size_t)n * kGpRecord * 8), dest_bytes = up64((size_t)n * 4);
    if ((rc = ctx->gp_work.reserve(words_bytes + grp_bytes + bound_bytes + rec_bytes + dest_bytes + DsWork::bytes(n_tiles, n_bounds))) ||
        (rc = ctx->gp_table.reserve((size_t)cap * 8)) || (rc = ctx->gp_cell.reserve((size_t)extent * 4))) return rc;
    uint8_t* w = ctx->gp_work.as<uint8_t>();
    uint32_t* d_words = reinterpret_cast<uint32_t*>(w); w += words_bytes;
    uint16_t* d_grp = reinterpret_cast<uint16_t*>(w); w += grp_bytes;
    GpBound* d_bound = reinterpret_cast<GpBound*>(w); w += bound_bytes;
    unsigned long long* d_rec = reinterpret_cast<unsigned long long*>(w); w += rec_bytes;
    uint32_t* d_dest = reinterpret_cast<uint32_t*>(w); w += dest_bytes;
    const DsWork W(w, n_tiles, n_bounds);
    unsigned long long* d_tbl = ctx->gp_table.as<unsigned long long>();
    uint32_t* d_cell = ctx->gp_cell.as<uint32_t>();

    // (host arrays the copies below read or write -- rel and run through the launcher's: ours, alive until the wait)
    std::vector<uint16_t> grp16(n);
    std::vector<GpBound> bounds(n_groups);
    std::vector<uint64_t> rel(n_bounds), run(n_bounds, 0);
    std::vector<unsigned long long> rec((size_t)n * kGpRecord);
    for (uint32_t i = 0; i < n; ++i) grp16[i] = (uint16_t)h_group[i];          // (a label is below n_groups <= 65 535)
    for (uint32_t c = 0; c < n_groups; ++c) bounds[c] = GpBound{in_min[c], out_max[c]};
    SPSP_HIP(hipMemsetAsync(d_words, 0, kGpWords * 4, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(d_grp, grp16.data(), (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(d_bound, bounds.data(), (size_t)n_groups * sizeof(GpBound), hipMemcpyHostToDevice, ctx->stream));
    // 1. h per entry
    if ((rc = prevalence_fill_table(ctx, has_hi, d_mn, d_lo, d_hi, h_sk_off, n, 0, false, d_words))) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    const uint64_t* d_off = ctx->pv_off.as<uint64_t>();
    const uint32_t* d_hold = ctx->pv_hold.as<uint32_t>();
    const SortedKeys K{d_mn, d_lo, d_hi};
    // 2. h_c per entry
    SPSP_HIP(hipMemsetAsync(d_tbl, 0, (size_t)cap * 8, ctx->stream));
    const uint32_t gx = (uint32_t)((all_keys + kGpThreads - 1) / kGpThreads);
    if (has_hi) {
        hipLaunchKernelGGL(k_gp_count<true>, dim3(gx), dim3(kGpThreads), 0, ctx->stream, K, d_off, n, (const uint16_t*)d_grp, d_tbl, log2cap, d_words);
        hipLaunchKernelGGL(k_gp_read<true>, dim3(gx), dim3(kGpThreads), 0, ctx->stream, K, d_off, n, (const uint16_t*)d_grp, (const GpBound*)d_bound, d_hold,
                           (const unsigned long long*)d_tbl, log2cap, d_cell, d_words);
    } else {
        hipLaunchKernelGGL(k_gp_count<false>, dim3(gx), dim3(kGpThreads), 0, ctx->stream, K, d_off, n, (const uint16_t*)d_grp, d_tbl, log2cap, d_words);
        hipLaunchKernelGGL(k_gp_read<false>, dim3(gx), dim3(kGpThreads), 0, ctx->stream, K, d_off, n, (const uint16_t*)d_grp, (const GpBound*)d_bound, d_hold,
                           (const unsigned long long*)d_tbl, log2cap, d_cell, d_words);
    }
    // 3. the records
    hipLaunchKernelGGL(k_gp_rows, dim3(n), dim3(kGpThreads), 0, ctx->stream, (const uint32_t*)d_cell, d_off, d_rec);
    SPSP_HIP(hipGetLastError());
    // 4. the markers' runs, sketch by sketch
    ctx->h_scalar[kHsGpTotal] = 0;
    if (want_markers) {
        if ((rc = ctx->gp_t_mn.reserve((size_t)all_keys * 4 + 64)) || (rc = ctx->gp_t_lo.reserve((size_t)all_keys * 8 + 64)) ||
            (has_hi && (rc = ctx->gp_t_hi.reserve((size_t)all_keys * 8 + 64)))) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        for (uint32_t i = 0; i < n_bounds; ++i) rel[i] = h_sk_off[i] - first;
        // kept: the entries that claimed their cell and whose cell is a marker.  The band 0 .. 0x7fffffff never cuts: it is tested on
        // the word's low 31 bits, and the flag bits sit inside them (only kGpClaim lies above) -- every value passes
        if ((rc = ds_flag_compact_launch(ctx, W, has_hi, d_mn + first, d_lo + first, has_hi ? d_hi + first : nullptr, d_cell + first, (uint32_t)all_keys, 0u,
                                         0x7fffffffu, kGpClaim | kGpMarker, rel.data(), n_bounds, ctx->gp_t_mn.as<uint32_t>(), ctx->gp_t_lo.as<uint64_t>(),
                                         has_hi ? ctx->gp_t_hi.as<uint64_t>() : nullptr, ctx->h_scalar + kHsGpTotal, run.data()))) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
    }
    SPSP_HIP(hipMemcpyAsync(ctx->h_scalar + kHsGpBad, d_words, 16, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(rec.data(), d_rec, rec.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the wait
    if ((uint32_t)ctx->h_scalar[kHsGpBad]) {
        set_error("sketch keys must be strictly increasing by (minimizer, kmer_hi, kmer_lo)");
        zero_results(rows, n_groups, members, n, marker_off);
        return SPSP_ERR_ARG;
    }
    if (ctx->h_scalar[kHsGpBad] >> 32 || (uint32_t)ctx->h_scalar[kHsGpCell]) {
        set_error("groups: a probe sequence went round its table (the key arrays changed during the call?)");
        zero_results(rows, n_groups, members, n, marker_off);
        return SPSP_ERR_ARG;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long* r = rec.data() + (size_t)i * kGpRecord;
        if (members) { members[i].core = r[0]; members[i].exclusive = r[1]; members[i].marker = r[2]; }
        spsp_group_row& g = rows[h_group[i]];
        g.present += r[3]; g.core += r[4]; g.exclusive += r[5]; g.marker += r[6];
    }
    if (!want_markers) return SPSP_OK;
    // 5. every group's region: its members' runs in list order; a region made of more than one run is sorted
    const uint64_t total = run[n];
    marker_off[0] = 0;
    for (uint32_t c = 0; c < n_groups; ++c) marker_off[c + 1] = marker_off[c] + rows[c].marker;
    if (marker_off[n_groups] != total) {
        set_error("groups: the marker runs (%llu keys) are not the groups' marker counts (%llu)", (unsigned long long)total, (unsigned long long)marker_off[n_groups]);
        zero_results(rows, n_groups, members, n, marker_off);
        return SPSP_ERR_ARG;
    }
    if (total == 0) return SPSP_OK;
    std::vector<uint32_t> dest(n), at(n_groups), runs(n_groups, 0);
    for (uint32_t c = 0; c < n_groups; ++c) at[c] = (uint32_t)marker_off[c];
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = h_group[i], len = (uint32_t)(run[i + 1] - run[i]);
        dest[i] = at[c];
        at[c] += len;
        if (len) ++runs[c];
    }
    if ((rc = ctx->gp_mn.reserve((size_t)total * 4 + 64)) || (rc = ctx->gp_lo.reserve((size_t)total * 8 + 64)) ||
        (has_hi && (rc = ctx->gp_hi.reserve((size_t)total * 8 + 64)))) { zero_results(rows, n_groups, members, n, marker_off); return rc; }
    uint32_t* o_mn = ctx->gp_mn.as<uint32_t>();
    uint64_t *o_lo = ctx->gp_lo.as<uint64_t>(), *o_hi = has_hi ? ctx->gp_hi.as<uint64_t>() : nullptr;
    *out_mn = o_mn; *out_lo = o_lo; *out_hi = o_hi;
    SPSP_HIP(hipMemcpyAsync(d_dest, dest.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (has_hi) hipLaunchKernelGGL(k_gp_regroup<true>, dim3(n), dim3(kGpThreads), 0, ctx->stream, (const uint32_t*)ctx->gp_t_mn.as<uint32_t>(),
                                   (const uint64_t*)ctx->gp_t_lo.as<uint64_t>(), (const uint64_t*)ctx->gp_t_hi.as<uint64_t>(), (const uint64_t*)W.off_out,
                                   (const uint32_t*)d_dest, (uint32_t)total, o_mn, o_lo, o_hi);
    else hipLaunchKernelGGL(k_gp_regroup<false>, dim3(n), dim3(kGpThreads), 0, ctx->stream, (const uint32_t*)ctx->gp_t_mn.as<uint32_t>(),
                            (const uint64_t*)ctx->gp_t_lo.as<uint64_t>(), (const uint64_t*)nullptr, (const uint64_t*)W.off_out, (const uint32_t*)d_dest,
                            (uint32_t)total, o_mn, o_lo, (uint64_t*)nullptr);
    SPSP_HIP(hipGetLastError());
    std::vector<std::pair<uint32_t, uint32_t>> segs;
    for (uint32_t c = 0; c < n_groups; ++c)
        if (runs[c] > 1) segs.push_back({(uint32_t)marker_off[c], (uint32_t)rows[c].marker});
    // (the compaction's output has been moved by then, in stream order: it is the sort's scratch; `dest` lives until the wait)
    if ((rc = big_sort_segments(ctx, has_hi, o_mn, o_lo, o_hi, ctx->gp_t_mn.as<uint32_t>(), ctx->gp_t_lo.as<uint64_t>(),
                                has_hi ? ctx->gp_t_hi.as<uint64_t>() : nullptr, segs))) { zero_results(rows, n_groups, members, n, marker_off); return rc; }
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // (the sort's own wait where it ran; the move's where no region needed it)
    return SPSP_OK;
}

// spsp_groups_files behind its argument checks: the labels read, the sketches loaded (spsp_host.cpp), decoded (and brought down to
// the common rate), the groups pass, the two CSVs and, on request, one marker sketch per group with the list of them
static int groups_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, const char* labels_path, int precision, uint32_t num, uint32_t den,
                        uint32_t onum, uint32_t oden, bool write_markers, const char* out_prefix, int chatter, double rate,
                        std::vector<spsp_group_row>* rows, std::vector<spsp_group_member_row>* members) {
    int rc;
    uint8_t* text_in = nullptr; uint64_t text_len = 0;
    if ((rc = spsp_read_file_host(labels_path, &text_in, &text_len))) return rc;
    std::vector<uint32_t> group(n);
    uint32_t G = 0;
    char* names_blob = nullptr; uint64_t names_len = 0;
    rc = spsp_groups_labels_host((const char*)text_in, text_len, n, group.data(), &G, &names_blob, &names_len);
    spsp_free(text_in);
    if (rc) { const std::string why = spsp_last_error(); set_error("'%s': %s", labels_path, why.c_str()); return rc; }
    const std::string names_own(names_blob, names_len);
    spsp_free(names_blob);
    std::vector<const char*> gname(G);
    { const char* p = names_own.c_str(); for (uint32_t c = 0; c < G; ++c) { gname[c] = p; p += strlen(p) + 1; } }
    if ((rc = spsp_groups_bounds_host(group.data(), n, G, num, den, onum, oden, nullptr, nullptr, nullptr))) return rc;

    FilesRun run(ctx, paths, n, chatter);
    rc = run.load(rate);
    if (!rc) rc = run.refuse_k_eq_m(rc, "groups are");
    double out_rate = run.L.ds_rate;
    if (!rc && write_markers) rc = sketches_out_rate(run.L, paths, n, &out_rate);
    if ((rc = run.begin(rc))) return rc;
    std::vector<uint64_t> moff((size_t)G + 1, 0);
    rows->assign(G, spsp_group_row{});
    members->assign(n, spsp_group_member_row{});
    const DecodedKeys& keys = run.keys;
    uint32_t* d_mn = nullptr; uint64_t *d_lo = nullptr, *d_hi = nullptr;
    rc = run.decode();
    if (!rc) rc = groups_device_impl(ctx, keys.k, keys.mn, keys.lo, keys.hi, keys.sk_off.data(), n, group.data(), G, num, den, onum, oden, rows->data(),
                                     members->data(), write_markers, &d_mn, &d_lo, &d_hi, moff.data());
    HostKeys got;
    if (!rc) rc = fetch_keys(ctx, keys.k, d_mn, d_lo, d_hi, write_markers ? moff[G] : 0, &got);
    const double t1 = run.end();
    if (rc) return rc;
    char* text = nullptr; uint64_t len = 0;
    if ((rc = spsp_groups_csv_host(rows->data(), G, gname.data(), precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_groups.csv.gz", t1))) return rc;
    const double t2 = now_s();
    if ((rc = spsp_groups_members_csv_host(members->data(), n, paths, group.data(), run.card.data(), rows->data(), G, gname.data(), precision, &text, &len))) return rc;
    if ((rc = write_csv_gz(ctx, text, len, out_prefix, "_members.csv.gz", t2))) return rc;
    if (write_markers) {
        const std::string list_path = std::string(out_prefix) + "_markers.txt";
        const auto name_of = [&](uint32_t c) { return std::string(out_prefix) + "_markers_" + std::to_string(c) + ".gz"; };
        if ((rc = write_key_sketches(keys.k, keys.m, out_rate, got, moff.data(), G, name_of, list_path.c_str()))) return rc;
    }
    if (chatter) {
        uint64_t core = 0, excl = 0, mark = 0;
        for (const spsp_group_row& r : *rows) { core += r.core; excl += r.exclusive; mark += r.marker; }
        printf("%u sketch(es) in %u group(s): %llu core, %llu exclusive and %llu marker key(s) over the groups\n", n, G, (unsigned long long)core,
               (unsigned long long)excl, (unsigned long long)mark);
        say_common_rate(run.L, n);
        fflush(stdout);
    }
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_groups_device(spsp_ctx* ctx, uint32_t k, const void* d_minimizer, const void* d_kmer_lo, const void* d_kmer_hi, const uint64_t* h_sk_off,
                                  uint32_t n, const uint32_t* h_group, uint32_t n_groups, uint32_t num, uint32_t den, uint32_t onum, uint32_t oden,
                                  spsp_group_row* rows, spsp_group_member_row* members, int want_markers, void** d_out_minimizer, void** d_out_kmer_lo,
                                  void** d_out_kmer_hi, uint64_t* marker_off) {
    if (d_out_minimizer) *d_out_minimizer = nullptr;
    if (d_out_kmer_lo) *d_out_kmer_lo = nullptr;
    if (d_out_kmer_hi) *d_out_kmer_hi = nullptr;
    if (!ctx || !h_sk_off || !h_group || !rows || (want_markers && (!d_out_minimizer || !d_out_kmer_lo || !d_out_kmer_hi || !marker_off))) {
        set_error("NULL argument");
        return SPSP_ERR_ARG;
    }
    SPSP_HIP(hipSetDevice(ctx->device));
    uint32_t* mn = nullptr; uint64_t *lo = nullptr, *hi = nullptr;
    const int rc = groups_device_impl(ctx, k, (const uint32_t*)d_minimizer, (const uint64_t*)d_kmer_lo, (const uint64_t*)d_kmer_hi, h_sk_off, n, h_group, n_groups,
                                      num, den, onum, oden, rows, members, want_markers != 0, &mn, &lo, &hi, marker_off);
    if (rc || !want_markers) return rc;
    *d_out_minimizer = mn; *d_out_kmer_lo = lo; *d_out_kmer_hi = hi;
    return SPSP_OK;
}

extern "C" int spsp_groups_files(spsp_ctx* ctx, const char* const* paths, uint32_t n, const char* labels_path, int precision, uint32_t num, uint32_t den,
                                 uint32_t onum, uint32_t oden, int write_markers, const char* out_prefix, int chatter, double rate, spsp_group_row** rows,
                                 spsp_group_member_row** members, uint32_t* n_groups) {
    if (rows) *rows = nullptr;
    if (members) *members = nullptr;
    if (n_groups) *n_groups = 0;
    if (!ctx || !paths || !labels_path || !out_prefix) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    if (n == 0 || n > 65535) { set_error("groups take 1 .. 65535 sketches (n = %u)", n); return SPSP_ERR_ARG; }
    int rc;
    SPSP_HIP(hipSetDevice(ctx->device));
    std::vector<spsp_group_row> got;
    std::vector<spsp_group_member_row> mem;
    if ((rc = groups_files(ctx, paths, n, labels_path, precision, num, den, onum, oden, write_markers != 0, out_prefix, chatter, rate, &got, &mem))) return rc;
    if (n_groups) *n_groups = (uint32_t)got.size();
    if (rows && (rc = give_rows(got, rows))) return rc;
    if (members && (rc = give_rows(mem, members))) { if (rows) { free(*rows); *rows = nullptr; } return rc; }
    return SPSP_OK;
}
