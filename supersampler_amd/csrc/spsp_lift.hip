// Raw coordinates on the GPU: kept-base indices lifted to positions among the sequence characters of the text the user holds (not
// in the reference, which has no record passes).  The rule is in include/spsp.h ("raw coordinates"); this file is its device form.
//
// The map is a select over the kept bases followed by a rank over the sequence characters, both over the raw text, which is cut
// into the ingest's tiles: 4 KiB, a lane per 16-byte chunk.  Four kinds of launch, ordered by the stream:
//   k_lf_tiles    per tile: the line-state transform (FASTA: does the tile end inside a header line; FASTQ: its newlines mod 4,
//                 so the line phase is additive), and per state the tile may be entered in the kept bases, the sequence
//                 characters and the record starts, 16 bits each in one 64-bit word per state
//   k_lf_scan     one workgroup: every tile's entry state and its prefixes K (kept), S (sequence), R (record starts)
//   k_lf_answer   a workgroup per tile: its queries are those with P[t] <= v < P[t + 1], found by two binary searches over the
//                 uploaded values (a tile that holds none of the counted kind skips even those; one without queries leaves).
//                 The others rebuild the chunks' masks, scan the chunks' counts into LDS, and a lane per query searches the
//                 256 prefixes, finds its bit in the chunk's mask by popcounts and counts the sequence bits below it.
//                 Run over K for the bases (-> sequence rank and record of every query), then over R for those records'
//                 starts (the same select, over the newlines that begin a record; a lane per START of the tile, which
//                 answers the first query of its record), and once more over R for every record where the lengths are asked
//   k_lf_finish   a lane per query: rank less its record's start (found by a search for its record's first query); a lane
//                 per record: the difference of two starts
// Tiles with no kept base give equal entries in K: the search is each tile's own half-open range, so such a tile has none and a
// query goes to the tile that holds its base.  Loads are guarded by n_text; every store is a lane's own query or a thread 0's own
// tile: no atomics, plain vector stores.  Work is balanced by input bytes, not by queries.
//
// The byte classification is this unit's own copy of the ingest's few helpers (spsp_ingest.hip stays as measured).
#include <algorithm>

#include "spsp_device.h"
#include "spsp_internal.h"

namespace spsp {

namespace {

static_assert(kLfThreads * kLfChunk == kLfTile && kLfTile <= 0xffffu && kLfChunk == 16, "a lane per 16-byte chunk; a tile's counts fit 16 bits");
constexpr int kLfWaves = kLfThreads / 64;

// 0x80 in every byte of v that is zero (exact); the four 0x80 flags of a word -> 4 bits (byte 0 -> bit 0)
__device__ __forceinline__ uint32_t lf_zero_bytes(uint32_t v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu); }
__device__ __forceinline__ uint32_t lf_flags(uint32_t z) { return (((z >> 7) * 0x01020408u) >> 24) & 0xFu; }
// 0x80 where the byte is one of ACGTacgt (the ingest's rule: case folded, the letter of the 2-bit code (c >> 1) & 3 compared)
__device__ __forceinline__ uint32_t lf_base_bytes(uint32_t w) {
    const uint32_t expect = __builtin_amdgcn_perm(0u, 0x47544341u, (w >> 1) & 0x03030303u);
    return lf_zero_bytes((w & 0xDFDFDFDFu) ^ expect);
}
// 0x80 where the byte is 0x21 .. 0x7e: the low seven bits reach 0x80 with 0x5f added, are not 0x7f, and bit 7 is clear
__device__ __forceinline__ uint32_t lf_graph_bytes(uint32_t w) {
    const uint32_t low = w & 0x7F7F7F7Fu;
    return (low + 0x5F5F5F5Fu) & ~(low + 0x01010101u) & ~w & 0x80808080u;
}

// a lane's 16 bytes as masks (bit j: byte j), bytes behind the text's end being nothing
struct LfChunk {
    uint32_t base;          // one of ACGTacgt
    uint32_t seq;           // 0x21 .. 0x7e
    uint32_t nl;            // '\n'
    uint32_t start_after;   // '\n', and the byte behind it exists and begins a record if its line may: FASTA '>' or 0xFF; FASTQ neither '\n' nor '\r'
};

template <bool FQ>
__device__ __forceinline__ LfChunk lf_load(const uint8_t* __restrict__ text, uint64_t n, uint64_t p0) {
    const uint32_t valid = p0 >= n ? 0u : (uint32_t)((n - p0) < (uint64_t)kLfChunk ? (n - p0) : (uint64_t)kLfChunk);
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    if (valid == kLfChunk) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + p0);
        b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
    } else {
        for (uint32_t j = 0; j < valid; ++j) b[j >> 2] |= (uint32_t)text[p0 + j] << (8u * (j & 3u));
    }
    const uint32_t in_mask = (1u << valid) - 1u;           // (valid <= 16)
    uint32_t base = 0, seq = 0, nl = 0, cand = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t w = b[d];
        base |= lf_flags(lf_base_bytes(w)) << (4 * d);
        seq |= lf_flags(lf_graph_bytes(w)) << (4 * d);
        const uint32_t is_nl = lf_zero_bytes(w ^ 0x0A0A0A0Au);
        nl |= lf_flags(is_nl) << (4 * d);
        if (FQ) cand |= lf_flags(is_nl | lf_zero_bytes(w ^ 0x0D0D0D0Du)) << (4 * d);   // (inverted below)
        else cand |= lf_flags(lf_zero_bytes(w ^ 0x3E3E3E3Eu) | lf_zero_bytes(w ^ 0xFFFFFFFFu)) << (4 * d);
    }
    if (FQ) cand = ~cand;
    cand &= in_mask;
    LfChunk c;
    c.base = base & in_mask; c.seq = seq & in_mask; c.nl = nl & in_mask;
    uint32_t next = 0;                                     // the byte behind the chunk, looked at only behind a newline in byte 15
    if ((c.nl >> 15) && p0 + kLfChunk < n) {
        const uint32_t f = text[p0 + kLfChunk];
        next = FQ ? (f != '\n' && f != '\r') : (f == '>' || f == 0xFFu);
    }
    c.start_after = c.nl & ((cand >> 1) | (next << 15));
    return c;
}

// The line state.  FASTA: 0 a data line, 1 a line that begins a record; a span's transform is 0 (no newline: identity) or
// 2 | the state behind its last newline.  FASTQ: the line's number mod 4; a span's transform is its newlines, added mod 4.
template <bool FQ>
__device__ __forceinline__ uint32_t lf_compose(uint32_t a, uint32_t b) { return FQ ? a + b : (b ? b : a); }   // a first, then b
template <bool FQ>
__device__ __forceinline__ uint32_t lf_transform(const LfChunk& c) {
    if (FQ) return __popc(c.nl);
    return c.nl ? 2u | ((c.start_after >> (31 - __clz(c.nl))) & 1u) : 0u;
}
// the state a span is entered in: the tile's entry state behind the transform of what lies in front of the span in the tile
template <bool FQ>
__device__ __forceinline__ uint32_t lf_state(uint32_t entry, uint32_t pre) { return FQ ? (entry + pre) & 3u : (pre ? pre & 1u : entry); }

// FASTA's composition as the += of the shared wave scan (lanes below arrive on the right)
struct LfFa { uint32_t t; };
__device__ __forceinline__ LfFa& operator+=(LfFa& p, const LfFa& q) { p.t = p.t ? p.t : q.t; return p; }

// the transform of the threads in front of this one, composed; `total`: of all of them.  The waves' sums pass through s_wave
// (WAVES words) with one barrier, as the scans of spsp_device.h have it
template <bool FQ, int WAVES>
__device__ __forceinline__ uint32_t lf_block_pre(uint32_t t, uint32_t lane, uint32_t wid, uint32_t* s_wave, uint32_t& total) {
    if (FQ) return block_prefix_excl<WAVES>(t, lane, wid, s_wave, total);
    const uint32_t incl = wave_prefix_incl(LfFa{t}, lane).t;
    if (lane == 63u) s_wave[wid] = incl;
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) { if (w < wid) pre = lf_compose<false>(pre, s_wave[w]); all = lf_compose<false>(all, s_wave[w]); }
    uint32_t below = __shfl_up(incl, 1);
    if (lane == 0u) below = 0u;
    total = all;
    return lf_compose<false>(pre, below);
}

// a chunk walked from state st: the kept bases, the sequence characters, the newlines that begin a record.  The bytes between
// two newlines share their line's state, so the walk is over the (rare) newlines
struct LfWalk { uint32_t keep, seq, rs; };
template <bool FQ>
__device__ __forceinline__ LfWalk lf_walk(const LfChunk& c, uint32_t st) {
    LfWalk w{0u, 0u, 0u};
    uint32_t from = 0, rem = c.nl;
    while (rem) {
        const uint32_t j = __ffs(rem) - 1;
        rem &= rem - 1;
        const uint32_t span = ((2u << j) - 1u) & ~((1u << from) - 1u);
        if (FQ ? st == 1u : st == 0u) { w.keep |= c.base & span; w.seq |= c.seq & span; }
        const uint32_t sa = (c.start_after >> j) & 1u;
        if (FQ) { st = (st + 1u) & 3u; if (st == 0u) w.rs |= sa << j; }
        else { st = sa; w.rs |= sa << j; }
        from = j + 1;
    }
    const uint32_t span = 0xFFFFu & ~((1u << from) - 1u);
    if (FQ ? st == 1u : st == 0u) { w.keep |= c.base & span; w.seq |= c.seq & span; }
    return w;
}

// what a tile is to the scan: its transform, and per entry state (FASTA 0..1, FASTQ 0..3) kept | sequence << 16 | starts << 32
struct LfTile { uint32_t t, spare; unsigned long long v[4]; };
struct LfSum4 { unsigned long long v[4]; };
__device__ __forceinline__ LfSum4& operator+=(LfSum4& p, const LfSum4& q) { p.v[0] += q.v[0]; p.v[1] += q.v[1]; p.v[2] += q.v[2]; p.v[3] += q.v[3]; return p; }
struct LfSum { unsigned long long k, s, r; };             // kept bases, sequence characters, record starts
__device__ __forceinline__ LfSum& operator+=(LfSum& p, const LfSum& q) { p.k += q.k; p.s += q.s; p.r += q.r; return p; }
__device__ __forceinline__ LfSum operator-(LfSum p, const LfSum& q) { p.k -= q.k; p.s -= q.s; p.r -= q.r; return p; }
__device__ __forceinline__ LfSum lf_unpack(unsigned long long v) { return LfSum{v & 0xffffull, (v >> 16) & 0xffffull, (v >> 32) & 0xffffull}; }
struct LfCnt { uint32_t sel, seq, rs; };
__device__ __forceinline__ LfCnt& operator+=(LfCnt& p, const LfCnt& q) { p.sel += q.sel; p.seq += q.seq; p.rs += q.rs; return p; }
__device__ __forceinline__ LfCnt operator-(LfCnt p, const LfCnt& q) { p.sel -= q.sel; p.seq -= q.seq; p.rs -= q.rs; return p; }

__device__ __forceinline__ bool lf_is_fastq(const uint8_t* __restrict__ text, uint64_t n) { return n != 0 && text[0] == '@'; }   // (uniform)

template <bool FQ>
__device__ __forceinline__ void lf_tiles_body(const uint8_t* __restrict__ text, uint64_t n, LfTile* __restrict__ tiles, uint32_t* s_w, LfSum4* s_tot) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const LfChunk c = lf_load<FQ>(text, n, (uint64_t)blockIdx.x * kLfTile + (uint64_t)threadIdx.x * kLfChunk);
    uint32_t tile_t;
    const uint32_t pre = lf_block_pre<FQ, kLfWaves>(lf_transform<FQ>(c), lane, wid, s_w, tile_t);
    LfSum4 me{{0ull, 0ull, 0ull, 0ull}};
#pragma unroll
    for (uint32_t e = 0; e < (FQ ? 4u : 2u); ++e) {
        if (!FQ && e == 1u && pre) { me.v[1] = me.v[0]; break; }   // behind the tile's first newline the entry state is forgotten
        const LfWalk w = lf_walk<FQ>(c, lf_state<FQ>(e, pre));
        me.v[e] = (unsigned long long)__popc(w.keep) | ((unsigned long long)__popc(w.seq) << 16) | ((unsigned long long)__popc(w.rs) << 32);
    }
    const LfSum4 all = block_sum<kLfWaves>(me, s_tot);
    if (threadIdx.x == 0) tiles[blockIdx.x] = LfTile{FQ ? tile_t & 3u : tile_t, 0u, {all.v[0], all.v[1], all.v[2], all.v[3]}};
}

__global__ __launch_bounds__(kLfThreads) void k_lf_tiles(const uint8_t* __restrict__ text, uint64_t n, LfTile* __restrict__ tiles) {
    __shared__ uint32_t s_w[kLfWaves];
    __shared__ LfSum4 s_tot[kLfWaves];
    if (lf_is_fastq(text, n)) lf_tiles_body<true>(text, n, tiles, s_w, s_tot);
    else lf_tiles_body<false>(text, n, tiles, s_w, s_tot);
}

// One workgroup of 512 (its three 64-bit sums and both formats' bodies do not fit the 128 registers a lane of 1 024 gets), a lane
// owning four consecutive tiles per round as in the ingest's scan: entry[t], and K, S, R [0 .. n_tiles]
constexpr int kLfScanTiles = 4, kLfScanThreads = 512, kLfScanWaves = kLfScanThreads / 64;
template <bool FQ>
__device__ __forceinline__ void lf_scan_body(const LfTile* __restrict__ tiles, uint64_t n_tiles, uint32_t* __restrict__ entry, unsigned long long* __restrict__ K,
                                             unsigned long long* __restrict__ S, unsigned long long* __restrict__ R, uint32_t* s_t, LfSum* s_sum, uint32_t* c_t, LfSum* c_sum) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    if (t == 0) { *c_t = FQ ? 0u : 3u; *c_sum = LfSum{0ull, 0ull, 0ull}; }   // FASTA: line 0 begins a record whatever it holds; FASTQ: line 0
    __syncthreads();
    for (uint64_t base = 0; base < n_tiles; base += (uint64_t)kLfScanThreads * kLfScanTiles) {   // (uniform)
        const uint64_t i0 = base + (uint64_t)t * kLfScanTiles;
        uint32_t mt[kLfScanTiles], tl = 0;                 // the transforms first: which of a tile's words counts is known behind their scan
#pragma unroll
        for (int u = 0; u < kLfScanTiles; ++u) {
            mt[u] = i0 + u < n_tiles ? tiles[i0 + u].t : 0u;
            tl = lf_compose<FQ>(tl, mt[u]);
        }
        uint32_t tall;
        const uint32_t pre = lf_block_pre<FQ, kLfScanWaves>(tl, lane, wid, s_t, tall);
        uint32_t state = lf_compose<FQ>(*c_t, pre);        // (FASTA: always a constant, as the carry starts as one)
        uint32_t ent[kLfScanTiles];
        unsigned long long cnt[kLfScanTiles];              // kept | sequence << 16 | starts << 32 in the state the tile is entered in
        LfSum sum{0ull, 0ull, 0ull};
#pragma unroll
        for (int u = 0; u < kLfScanTiles; ++u) {
            ent[u] = FQ ? state & 3u : state & 1u;
            cnt[u] = i0 + u < n_tiles ? tiles[i0 + u].v[ent[u]] : 0ull;
            sum += lf_unpack(cnt[u]);
            state = lf_compose<FQ>(state, mt[u]);
        }
        LfSum all;
        LfSum run = block_prefix_excl<kLfScanWaves>(sum, lane, wid, s_sum, all);
        run += *c_sum;
#pragma unroll
        for (int u = 0; u < kLfScanTiles; ++u) {
            if (i0 + u < n_tiles) { entry[i0 + u] = ent[u]; K[i0 + u] = run.k; S[i0 + u] = run.s; R[i0 + u] = run.r; }
            run += lf_unpack(cnt[u]);
        }
        __syncthreads();
        if (t == 0) { *c_t = FQ ? (*c_t + tall) & 3u : lf_compose<false>(*c_t, tall); *c_sum += all; }
        __syncthreads();
    }
    if (t == 0) { K[n_tiles] = c_sum->k; S[n_tiles] = c_sum->s; R[n_tiles] = c_sum->r; }
}

__global__ __launch_bounds__(kLfScanThreads) void k_lf_scan(const uint8_t* __restrict__ text, uint64_t n, const LfTile* __restrict__ tiles, uint64_t n_tiles,
                                                  uint32_t* __restrict__ entry, unsigned long long* __restrict__ K, unsigned long long* __restrict__ S,
                                                  unsigned long long* __restrict__ R) {
    __shared__ uint32_t s_t[kLfScanWaves];
    __shared__ LfSum s_sum[kLfScanWaves];
    __shared__ uint32_t c_t;
    __shared__ LfSum c_sum;
    if (lf_is_fastq(text, n)) lf_scan_body<true>(tiles, n_tiles, entry, K, S, R, s_t, s_sum, &c_t, &c_sum);
    else lf_scan_body<false>(tiles, n_tiles, entry, K, S, R, s_t, s_sum, &c_t, &c_sum);
}

// The values a launch of the answer searches for, ascending.  kLfBases: q[i], a global kept-base index.  The two others name
// RECORDS, and record r >= 1 begins behind start r - 1 (record 0 begins with the text and is found in no tile).  kLfRecStarts:
// q[i], the record of query i as the first launch wrote it.  kLfAllStarts: record i + 1
enum LfAsk { kLfBases = 0, kLfRecStarts = 1, kLfAllStarts = 2 };
struct LfQueries {
    const unsigned long long* q; int ask;
    __device__ __forceinline__ unsigned long long operator()(uint32_t i) const { return ask == kLfAllStarts ? (unsigned long long)i + 1ull : q[i]; }
};
// the first i of [lo, n) whose value is v or more
__device__ __forceinline__ uint32_t lf_lower_bound(const LfQueries& Q, uint32_t lo, uint32_t n, unsigned long long v) {
    uint32_t hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (Q(mid) < v) lo = mid + 1u; else hi = mid; }
    return lo;
}

struct LfLds { uint32_t range[2], w[kLfWaves]; LfCnt cw[kLfWaves]; uint32_t sel[kLfThreads], seq[kLfThreads], rs[kLfThreads], mask[kLfThreads], rsm[kLfThreads]; };

// item `local` of the tile's selected kind (bases, or starts): the last chunk whose prefix is at most local holds it; its bit in the
// chunk's mask by popcounts of halves; -> the sequence characters and the record starts of the tile below that bit
__device__ __forceinline__ void lf_select(const LfLds& L, uint32_t local, uint32_t* seq_below, uint32_t* rs_below) {
    uint32_t lo = 0, hi = kLfThreads;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (L.sel[mid] <= local) lo = mid; else hi = mid; }
    uint32_t i = local - L.sel[lo], m = L.mask[lo] & 0xffffu, pos = 0;
#pragma unroll
    for (uint32_t width = 8; width; width >>= 1) {
        const uint32_t below = __popc(m & ((1u << width) - 1u));
        if (i >= below) { i -= below; m >>= width; pos += width; }
    }
    const uint32_t under = (1u << pos) - 1u;
    *seq_below = L.seq[lo] + __popc((L.mask[lo] >> 16) & under);
    *rs_below = L.rs[lo] + __popc(L.rsm[lo] & under);
}

// q_lo, q_hi: the tile's queries; P0, P1: its prefixes of the counted kind.  START: the counted kind is the record starts, else the
// kept bases.  Bases: a lane per query (below the tile's count: the two passes count alike).  Starts: a lane per START of the tile,
// which looks for the first query that names its record and answers that one alone -- every query of one record names the same
// start, so a lane per query would leave a record's 10^5 segment ends to the one workgroup that holds its start; the queries
// behind the first find it by a search of their own (k_lf_finish)
template <bool FQ, bool START>
__device__ __forceinline__ void lf_answer_body(const uint8_t* __restrict__ text, uint64_t n, uint32_t entry, unsigned long long P0, unsigned long long P1,
                                               unsigned long long S0, unsigned long long R0, const LfQueries& Q, uint32_t q_lo, uint32_t q_hi,
                                               unsigned long long* __restrict__ out_seq, unsigned long long* __restrict__ out_rec, LfLds& L) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const LfChunk c = lf_load<FQ>(text, n, (uint64_t)blockIdx.x * kLfTile + (uint64_t)tid * kLfChunk);
    uint32_t tile_t;
    const uint32_t pre = lf_block_pre<FQ, kLfWaves>(lf_transform<FQ>(c), lane, wid, L.w, tile_t);
    const LfWalk w = lf_walk<FQ>(c, lf_state<FQ>(entry, pre));
    const uint32_t sel = START ? w.rs : w.keep;
    const LfCnt ex = block_prefix_excl<kLfWaves>(LfCnt{(uint32_t)__popc(sel), (uint32_t)__popc(w.seq), (uint32_t)__popc(w.rs)}, lane, wid, L.cw);
    L.sel[tid] = ex.sel; L.seq[tid] = ex.seq; L.rs[tid] = ex.rs; L.mask[tid] = sel | (w.seq << 16); L.rsm[tid] = w.rs;
    __syncthreads();
    uint32_t seq_below, rs_below;
    if (START) {
        const uint32_t n_starts = (uint32_t)(P1 - P0);     // (at most a tile's bytes)
        for (uint32_t j = tid; j < n_starts; j += kLfThreads) {
            const unsigned long long r = P0 + j + 1ull;    // the record that begins behind the tile's start j
            const uint32_t q = lf_lower_bound(Q, q_lo, q_hi, r);
            if (q >= q_hi || Q(q) != r) continue;
            lf_select(L, j, &seq_below, &rs_below);
            out_seq[q] = S0 + seq_below;
        }
    } else {
        for (uint32_t q = q_lo + tid; q < q_hi; q += kLfThreads) {
            lf_select(L, (uint32_t)(Q(q) - P0), &seq_below, &rs_below);
            out_seq[q] = S0 + seq_below;
            out_rec[q] = R0 + rs_below;
        }
    }
}

__global__ __launch_bounds__(kLfThreads) void k_lf_answer(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ entry,
                                                          const unsigned long long* __restrict__ K, const unsigned long long* __restrict__ S,
                                                          const unsigned long long* __restrict__ R, LfQueries Q, uint32_t n_q, unsigned long long* __restrict__ out_seq,
                                                          unsigned long long* __restrict__ out_rec) {
    __shared__ LfLds L;
    const bool start = Q.ask != kLfBases;                  // (uniform, as everything up to the bodies)
    const unsigned long long* P = start ? R : K;
    const unsigned long long P0 = P[blockIdx.x], P1 = P[blockIdx.x + 1];
    if (P0 == P1) return;                                  // a tile that holds none of the counted kind holds no query
    const unsigned long long first = start ? 1ull : 0ull;  // start j begins record j + 1
    if (threadIdx.x == 0u) L.range[0] = lf_lower_bound(Q, 0u, n_q, P0 + first);
    if (threadIdx.x == 64u) L.range[1] = lf_lower_bound(Q, 0u, n_q, P1 + first);
    __syncthreads();
    const uint32_t q_lo = L.range[0], q_hi = L.range[1];
    if (q_lo >= q_hi) return;
    const uint32_t e = entry[blockIdx.x];
    const unsigned long long S0 = S[blockIdx.x], R0 = R[blockIdx.x];
    if (lf_is_fastq(text, n)) {
        if (start) lf_answer_body<true, true>(text, n, e, P0, P1, S0, R0, Q, q_lo, q_hi, out_seq, out_rec, L);
        else lf_answer_body<true, false>(text, n, e, P0, P1, S0, R0, Q, q_lo, q_hi, out_seq, out_rec, L);
    } else {
        if (start) lf_answer_body<false, true>(text, n, e, P0, P1, S0, R0, Q, q_lo, q_hi, out_seq, out_rec, L);
        else lf_answer_body<false, false>(text, n, e, P0, P1, S0, R0, Q, q_lo, q_hi, out_seq, out_rec, L);
    }
}

// a lane per query: its rank among the sequence characters less its record's start, which the start launch left with the FIRST
// query of that record (a search over the records the base launch wrote, ascending); a lane per record: the next record's start
// (the text's sequence characters behind the last record) less its own.  all_start[j]: where record j + 1 begins
__global__ __launch_bounds__(kLfThreads) void k_lf_finish(const unsigned long long* __restrict__ seq, const unsigned long long* __restrict__ rec,
                                                          const unsigned long long* __restrict__ rec_start, uint32_t n_q, unsigned long long* __restrict__ raw,
                                                          uint32_t* __restrict__ rec32, const unsigned long long* __restrict__ all_start, uint32_t n_len,
                                                          const unsigned long long* __restrict__ s_total, unsigned long long* __restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * kLfThreads + threadIdx.x;
    if (i < n_q) {
        const unsigned long long r = rec[i];
        raw[i] = seq[i] - (r ? rec_start[lf_lower_bound(LfQueries{rec, kLfRecStarts}, 0u, (uint32_t)i, r)] : 0ull);   // (at most i: the query's own)
        rec32[i] = (uint32_t)r;
    }
    if (i < n_len) len[i] = (i + 1 < n_len ? all_start[i] : *s_total) - (i ? all_start[i - 1] : 0ull);
}

}  // namespace

int records_lift_impl(spsp_ctx* ctx, const uint8_t* d_text, uint64_t n_text, uint64_t n_bases, const uint64_t* h_base, uint64_t n_q, uint64_t* raw, uint32_t* rec,
                      uint64_t* raw_length, uint32_t* n_rec) {
    int rc;
    const uint32_t cap = raw_length ? *n_rec : 0u;         // the records raw_length has room for
    *n_rec = 0;
    // refused before any launch
    if (((uintptr_t)d_text & 15u) != 0) { set_error("d_text must be 16-byte aligned"); return SPSP_ERR_ARG; }
    if (n_q > 0xfffffff0ull) { set_error("lift: too many positions for one call (%llu)", (unsigned long long)n_q); return SPSP_ERR_OVERFLOW; }
    for (uint64_t q = 1; q < n_q; ++q)
        if (h_base[q] < h_base[q - 1]) { set_error("lift: the base indices must not decrease (index %llu)", (unsigned long long)q); return SPSP_ERR_ARG; }
    if (n_q && n_bases == 0) { set_error("lift: %llu position(s) asked of a text without bases", (unsigned long long)n_q); return SPSP_ERR_ARG; }
    if (raw_length && cap == 0) { set_error("lift: raw_length asks for the record count the ingest gave (1 or more)"); return SPSP_ERR_ARG; }
    const uint64_t n_tiles = (n_text + kLfTile - 1) / kLfTile;
    if (n_tiles > 0x7fffffffull) { set_error("text too large for one call"); return SPSP_ERR_OVERFLOW; }
    if (n_q == 0 && !raw_length) return SPSP_OK;           // nothing is asked: nothing is launched (and no record is counted)
    const size_t nq = (size_t)n_q, nt1 = (size_t)n_tiles + 1;
    if ((rc = ctx->lf_tiles.reserve(nt1 * sizeof(LfTile))) || (rc = ctx->lf_entry.reserve(nt1 * 4)) || (rc = ctx->lf_pre.reserve(nt1 * 24)) ||
        (rc = ctx->lf_q.reserve((nq + 1) * 8)) || (rc = ctx->lf_work.reserve((nq + 1) * 24 + ((size_t)cap + 1) * 8)) ||
        (rc = ctx->lf_out.reserve((nq + 1) * 8 + ((size_t)cap + 1) * 8 + (nq + 1) * 4))) return rc;
    unsigned long long *K = ctx->lf_pre.as<unsigned long long>(), *S = K + nt1, *R = S + nt1;
    unsigned long long *d_q = ctx->lf_q.as<unsigned long long>();
    unsigned long long *d_seq = ctx->lf_work.as<unsigned long long>(), *d_rec = d_seq + (nq + 1), *d_start = d_rec + (nq + 1), *d_all = d_start + (nq + 1);
    unsigned long long *d_raw = ctx->lf_out.as<unsigned long long>(), *d_len = d_raw + (nq + 1);
    uint32_t* d_rec32 = reinterpret_cast<uint32_t*>(d_len + ((size_t)cap + 1));
    if (n_q) SPSP_HIP(hipMemcpyAsync(d_q, h_base, nq * 8, hipMemcpyHostToDevice, ctx->stream));   // the one upload
    // a query no tile answers (an index that is not below the text's bases: refused behind the wait) reads as rank 0 of record 0 in
    // the launches behind the first, not as what an earlier call left there
    if (n_q) SPSP_HIP(hipMemsetAsync(d_seq, 0, (nq + 1) * 24, ctx->stream));
    const bool timing = ctx->timing;
    if (timing) {
        for (hipEvent_t& e : ctx->lf_ev) if (!e) SPSP_HIP(hipEventCreate(&e));
        SPSP_HIP(hipEventRecord(ctx->lf_ev[0], ctx->stream));
    }
    if (n_tiles) {
        hipLaunchKernelGGL(k_lf_tiles, dim3((uint32_t)n_tiles), dim3(kLfThreads), 0, ctx->stream, d_text, n_text, ctx->lf_tiles.as<LfTile>());
        SPSP_HIP(hipGetLastError());
    }
    if (timing) SPSP_HIP(hipEventRecord(ctx->lf_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_lf_scan, dim3(1), dim3(kLfScanThreads), 0, ctx->stream, d_text, n_text, ctx->lf_tiles.as<LfTile>(), n_tiles, ctx->lf_entry.as<uint32_t>(), K, S, R);
    SPSP_HIP(hipGetLastError());
    if (timing) SPSP_HIP(hipEventRecord(ctx->lf_ev[2], ctx->stream));
    const uint32_t* d_entry = ctx->lf_entry.as<uint32_t>();
    if (n_tiles && n_q) {
        hipLaunchKernelGGL(k_lf_answer, dim3((uint32_t)n_tiles), dim3(kLfThreads), 0, ctx->stream, d_text, n_text, d_entry, K, S, R, LfQueries{d_q, kLfBases}, (uint32_t)n_q,
                           d_seq, d_rec);
        SPSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_lf_answer, dim3((uint32_t)n_tiles), dim3(kLfThreads), 0, ctx->stream, d_text, n_text, d_entry, K, S, R, LfQueries{d_rec, kLfRecStarts},
                           (uint32_t)n_q, d_start, (unsigned long long*)nullptr);
        SPSP_HIP(hipGetLastError());
    }
    if (n_tiles && cap > 1) {
        hipLaunchKernelGGL(k_lf_answer, dim3((uint32_t)n_tiles), dim3(kLfThreads), 0, ctx->stream, d_text, n_text, d_entry, K, S, R,
                           LfQueries{(const unsigned long long*)nullptr, kLfAllStarts}, cap - 1u, d_all, (unsigned long long*)nullptr);
        SPSP_HIP(hipGetLastError());
    }
    const uint32_t n_fin = std::max<uint32_t>((uint32_t)n_q, cap);
    hipLaunchKernelGGL(k_lf_finish, dim3((n_fin + kLfThreads - 1) / kLfThreads), dim3(kLfThreads), 0, ctx->stream, d_seq, d_rec, d_start, (uint32_t)n_q, d_raw, d_rec32, d_all,
                       cap, S + n_tiles, d_len);
    SPSP_HIP(hipGetLastError());
    if (timing) SPSP_HIP(hipEventRecord(ctx->lf_ev[3], ctx->stream));
    unsigned long long totals[2] = {0ull, 0ull};           // the text's kept bases and record starts
    SPSP_HIP(hipMemcpyAsync(&totals[0], K + n_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipMemcpyAsync(&totals[1], R + n_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n_q) SPSP_HIP(hipMemcpyAsync(raw, d_raw, nq * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n_q && rec) SPSP_HIP(hipMemcpyAsync(rec, d_rec32, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (raw_length) SPSP_HIP(hipMemcpyAsync(raw_length, d_len, (size_t)cap * 8, hipMemcpyDeviceToHost, ctx->stream));
    SPSP_HIP(hipStreamSynchronize(ctx->stream));           // the one wait
    if (timing)
        for (int i = 0; i < 3; ++i) { float ms = 0; SPSP_HIP(hipEventElapsedTime(&ms, ctx->lf_ev[i], ctx->lf_ev[i + 1])); ctx->lf_ms[i] += ms; }
    // refused behind the wait: what only the text's own counts can say
    if (totals[1] + 1ull > 0xfffffff0ull) { set_error("too many records for one call"); return SPSP_ERR_OVERFLOW; }
    *n_rec = (uint32_t)(totals[1] + 1ull);
    if (n_q && h_base[n_q - 1] >= n_bases) {
        set_error("lift: base index %llu is not below the %llu bases", (unsigned long long)h_base[n_q - 1], (unsigned long long)n_bases);
        return SPSP_ERR_ARG;
    }
    if (totals[0] != n_bases) {
        set_error("lift: the text holds %llu kept base(s), not the %llu it was called with", (unsigned long long)totals[0], (unsigned long long)n_bases);
        return SPSP_ERR_ARG;
    }
    if (raw_length && cap != *n_rec) { set_error("lift: the text holds %u record(s), raw_length has room for %u", *n_rec, cap); return SPSP_ERR_ARG; }
    return SPSP_OK;
}

}  // namespace spsp

using namespace spsp;

extern "C" int spsp_records_lift_device(spsp_ctx* ctx, const void* d_text, uint64_t n_text, uint64_t n_bases, const uint64_t* h_base, uint64_t n_q, uint64_t* raw,
                                        uint32_t* rec, uint64_t* raw_length, uint32_t* n_rec) {
    if (!ctx || !n_rec || (n_text && !d_text) || (n_q && (!h_base || !raw))) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    SPSP_HIP(hipSetDevice(ctx->device));
    return records_lift_impl(ctx, (const uint8_t*)d_text, n_text, n_bases, h_base, n_q, raw, rec, raw_length, n_rec);
}

extern "C" int spsp_lift_stage_ms(spsp_ctx* ctx, double* ms) {
    if (!ctx || !ms) { set_error("NULL argument"); return SPSP_ERR_ARG; }
    for (int i = 0; i < 3; ++i) { ms[i] = ctx->lf_ms[i]; ctx->lf_ms[i] = 0; }
    return SPSP_OK;
}
