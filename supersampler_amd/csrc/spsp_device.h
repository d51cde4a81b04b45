// Device-side primitives shared by the scan and compare kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spsp {

// XXH64 of one little-endian 64-bit word, seed 1312 -- the reference's
// Subsampler::unrevhash (SubSampler.cpp:64-67 -> include/xxhash64.h:100-150).
// Closed form for an 8-byte input: no stripe loop, one "remaining 8 bytes"
// round and the avalanche.  gfx950 has no 64x64 multiply; each `*` below is a
// few v_mul_lo_u32 / v_mul_hi_u32 / v_mad_u64_u32.
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

__device__ __forceinline__ uint64_t xxh64_u64(uint64_t x) {
    constexpr uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL,
                       P3 = 1609587929392839161ULL, P4 = 9650029242287828579ULL,
                       P5 = 2870177450012600261ULL;
    uint64_t h = 1312ULL + P5 + 8ULL;
    h ^= rotl64(x * P2, 31) * P1;
    h = rotl64(h, 27) * P1 + P4;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

// Reverse complement of a full 64-bit window of 32 bases (first base in the top
// two bits; A=0 C=1 T=2 G=3 so complement = code ^ 2): reverse the order of the
// 2-bit groups, then flip the high bit of each group.
__device__ __forceinline__ uint64_t rc_window64(uint64_t w) {
    uint64_t r = __brevll(w);
    r = ((r & 0x5555555555555555ULL) << 1) | ((r >> 1) & 0x5555555555555555ULL);
    return r ^ 0xAAAAAAAAAAAAAAAAULL;
}
__device__ __forceinline__ uint32_t rc_window32(uint32_t w) {
    uint32_t r = __brev(w);
    r = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
    return r ^ 0xAAAAAAAAu;
}
// reverse complement of an m-mer held in the low 2m bits (reference rcbc, utils.cpp:449-462)
__device__ __forceinline__ uint32_t rc_mmer32(uint32_t v, uint32_t m) { return rc_window32(v) >> (32 - 2 * m); }

// 16 ASCII bases -> 32 bits, first base in the two most significant bits.
// code = (c >> 1) & 3 (reference utils.cpp:13-16: A=0 C=1 T=2 G=3).
// Four bases per dword with ONE dot instruction: bytes & 0x06 hold 2*code, and v_dot4_u32_u8 with byte
// weights 64,16,4,1 (first base = lowest byte = most significant field) sums them into 2 * (b0<<6|b1<<4|b2<<2|b3).
// The factor 2 is carried through the shift-or merges and dropped by the last shift, so 16 bases cost
// 4 and + 4 dot4 + 4 merges (a 32-bit integer multiply, the previous form, is a quarter-rate instruction).
__device__ __forceinline__ uint32_t pack4x2(uint32_t d) {
    return __builtin_amdgcn_udot4(d & 0x06060606u, 0x01041040u, 0u, false);
}
__device__ __forceinline__ uint32_t pack16(uint4 v) {
    const uint32_t a = (pack4x2(v.x) << 8) | pack4x2(v.y);   // 2 * (first 8 bases)
    const uint32_t b = (pack4x2(v.z) << 8) | pack4x2(v.w);   // 2 * (last 8 bases)
    return (a << 15) | (b >> 1);
}

// The comparator's keys as gather and prevalence read them: concatenated arrays, every sketch sorted by (minimizer, kmer_hi, kmer_lo);
// off[j] = the first entry of sketch j.
struct SortedKeys { const uint32_t* mn; const uint64_t* lo; const uint64_t* hi; };

template <bool HAS_HI>
__device__ __forceinline__ bool keys_less(const SortedKeys& K, uint64_t i, uint32_t mn, uint64_t hi, uint64_t lo) {   // key i < (mn, hi, lo)
    const uint32_t a = K.mn[i];
    if (a != mn) return a < mn;
    if (HAS_HI) { const uint64_t h = K.hi[i]; if (h != hi) return h < hi; }
    return K.lo[i] < lo;
}

// the sketch that holds entry e: the last j in [j0, j1) with off[j] <= e (sketches without keys are stepped over)
__device__ __forceinline__ uint32_t sorted_sketch_of(const uint64_t* __restrict__ off, uint32_t j0, uint32_t j1, uint64_t e) {
    uint32_t a = j0, b = j1;                               // first j in [j0, j1] with off[j] > e
    while (a < b) { const uint32_t mid = a + ((b - a) >> 1); if (off[mid] <= e) a = mid + 1; else b = mid; }
    return a - 1;
}

// flag[0] |= 1 when entry e does not come strictly after e - 1 inside its sketch (sketches [j0, j1) own entries [off[j0], off[j1]))
template <bool HAS_HI>
__device__ __forceinline__ void sorted_check_order(const SortedKeys& K, const uint64_t* __restrict__ off, uint32_t j0, uint32_t j1, uint64_t e,
                                              uint32_t mn, uint64_t hi, uint64_t lo, uint32_t* __restrict__ flag) {
    if (e == off[j0] || keys_less<HAS_HI>(K, e - 1, mn, hi, lo)) return;
    if (e != off[sorted_sketch_of(off, j0, j1, e)]) atomicOr(flag, 1u);   // (the first key of a sketch may be anything)
}

// The prevalence table (spsp_prevalence.hip: one 64-bit word per slot, the claimer's entry number + 1 in the low half): a key's
// home slot in a table of 2^log2cap slots, and whether entry c holds the key (mn, hi, lo).  The fill, the read-back and the
// accumulation's transposition (spsp_accumulation.hip) walk the same probe sequence from the same home.
template <bool HAS_HI>
__device__ __forceinline__ uint64_t pv_home(uint32_t mn, uint64_t hi, uint64_t lo, uint32_t log2cap) {
    uint64_t h = xxh64_u64(lo + (uint64_t)(mn + 1u) * 0x9E3779B97F4A7C15ULL);
    if (HAS_HI) h = xxh64_u64(h ^ hi);
    return h >> (64u - log2cap);                           // (log2cap >= 1)
}

template <bool HAS_HI>
__device__ __forceinline__ bool pv_same(const SortedKeys& K, uint64_t c, uint32_t mn, uint64_t hi, uint64_t lo) {
    return K.lo[c] == lo && K.mn[c] == mn && (!HAS_HI || K.hi[c] == hi);
}

// The lookup of a key in a table the fill made from entries [first, first + n_index) of K: the probe sequence from the key's home
// up to the first free slot, or once round a table without one.  -> the claimer's entry number less `first`, or ~0: nobody holds
// the key.  The classification's probe pass and the depth pass's counting pass walk it.
template <bool HAS_HI>
__device__ __forceinline__ uint64_t pv_find(const SortedKeys& K, uint64_t first, uint32_t n_index, const unsigned long long* __restrict__ tbl, uint32_t log2cap,
                                            uint32_t mn, uint64_t hi, uint64_t lo) {
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t pos = pv_home<HAS_HI>(mn, hi, lo, log2cap);
    for (uint64_t probes = 0; probes <= mask; ++probes) {   // (a key nobody holds may go round a table without a free slot)
        const unsigned long long cur = tbl[pos];
        if ((uint32_t)cur == 0u) break;
        const uint64_t c = (uint64_t)((uint32_t)cur - 1u), at = c - first;
        if (at < n_index && pv_same<HAS_HI>(K, c, mn, hi, lo)) return at;   // (always inside: the index call filled this table from these entries)
        pos = (pos + 1ull) & mask;
    }
    return ~0ull;
}

// The order of two fractions x_a / u_a and x_b / u_b without a division: x_a * u_b against x_b * u_a as 128-bit products.
// > 0: a is the larger fraction, < 0: b, 0: equal (two different fractions that round to one double are still told apart).
// The neighbours pass orders a row's partners by it, the representatives pass a member's candidates.
__device__ __forceinline__ int fraction_cmp(unsigned long long x_a, unsigned long long u_a, unsigned long long x_b, unsigned long long u_b) {
    const unsigned long long lo_a = x_a * u_b, hi_a = __umul64hi(x_a, u_b), lo_b = x_b * u_a, hi_b = __umul64hi(x_b, u_a);
    if (hi_a != hi_b) return hi_a > hi_b ? 1 : -1;
    if (lo_a != lo_b) return lo_a > lo_b ? 1 : -1;
    return 0;
}

// The lock-free union-find over parent[0 .. n) that the cluster pass and the linkage tree share (spsp_cluster.hip says what it
// relies on: parent[x] <= x always, parent[x] == x only for a root, a hooked node never becomes a root again).
__device__ __forceinline__ uint32_t cl_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, whose parent word was just read as p; every second node on the way is handed to its grandparent
__device__ __forceinline__ uint32_t cl_find(uint32_t* __restrict__ parent, uint32_t x, uint32_t p) {
    while (p != x) {
        const uint32_t g = cl_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);                          // (never back to a farther ancestor, whoever else halves here)
        x = g;
        p = cl_load(parent + x);
    }
    return x;
}

__device__ __forceinline__ void cl_union(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
    uint32_t pa = cl_load(parent + a), pb = cl_load(parent + b);
    for (;;) {
        if (pa == pb) return;                              // two loads say "one tree already": the common case of a large component
        a = cl_find(parent, a, pa);
        b = cl_find(parent, b, pb);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return;
        a = was; pa = cl_load(parent + a);                 // hi was hooked by somebody else meanwhile: on from where it hangs now
        b = lo; pb = cl_load(parent + b);
    }
}

// ---- What the record passes share on the device (DESIGN "What the record passes share"): classify, taxonomy, depth, profile and the
// key-major build of the accumulation.  A wave is 64 lanes; every helper is called by all of them (uniform control flow).

// the wave's LDS words: what its lanes stored in front of this line is what they read behind it
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The sums a scan may run over besides a 32- or 64-bit count: small records of whole dwords with += and -, summed field by field.
struct ExSum { unsigned long long a; uint32_t b, c; };   // 16 bytes: bytes (or starts), runs, records kept (extract, split)
struct __attribute__((packed, aligned(4))) Sum64x32 { unsigned long long a; uint32_t b; };   // 12 bytes: a 64-bit and a 32-bit count at once
struct WnSum { unsigned long long bases, wins; };        // (windows)
struct Sum2 { uint32_t x, y; };                          // two counts scanned at once
__device__ __forceinline__ ExSum& operator+=(ExSum& p, const ExSum& q) { p.a += q.a; p.b += q.b; p.c += q.c; return p; }
__device__ __forceinline__ ExSum operator-(ExSum p, const ExSum& q) { p.a -= q.a; p.b -= q.b; p.c -= q.c; return p; }
__device__ __forceinline__ Sum64x32& operator+=(Sum64x32& p, const Sum64x32& q) { p.a += q.a; p.b += q.b; return p; }
__device__ __forceinline__ Sum64x32 operator-(Sum64x32 p, const Sum64x32& q) { p.a -= q.a; p.b -= q.b; return p; }
__device__ __forceinline__ WnSum& operator+=(WnSum& p, const WnSum& q) { p.bases += q.bases; p.wins += q.wins; return p; }
__device__ __forceinline__ WnSum operator-(WnSum p, const WnSum& q) { p.bases -= q.bases; p.wins -= q.wins; return p; }
__device__ __forceinline__ Sum2& operator+=(Sum2& p, const Sum2& q) { p.x += q.x; p.y += q.y; return p; }
__device__ __forceinline__ Sum2 operator-(Sum2 p, const Sum2& q) { p.x -= q.x; p.y -= q.y; return p; }

// v of the lane d below (UP) or of lane ^ d, a 32-bit shuffle per dword of T
template <bool UP, class T>
__device__ __forceinline__ T lane_get(T v, int d) {
    static_assert(sizeof(T) % 4 == 0 && __is_trivially_copyable(T), "whole dwords");
    if constexpr (__is_integral(T)) return UP ? __shfl_up(v, d) : __shfl_xor(v, d);
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
    for (uint32_t i = 0; i < sizeof(T) / 4; ++i) w[i] = UP ? __shfl_up(w[i], d) : __shfl_xor(w[i], d);
    __builtin_memcpy(&v, w, sizeof(T));
    return v;
}

// reductions over the wave: every lane gets the result
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += lane_get<false>(v, d);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
// the sum of v over the lanes up to and including this one
template <class T>
__device__ __forceinline__ T wave_prefix_incl(T v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T t = lane_get<true>(v, d); if ((int)lane >= d) v += t; }
    return v;
}

// ---- What the prefix sums share (DESIGN "What the prefix sums share").  A workgroup of WAVES waves, lane = threadIdx.x & 63 and
// wid = threadIdx.x >> 6 from the caller, s_wave: WAVES items of LDS.  Each has one barrier, behind the store to s_wave and in front
// of its reads: whoever stores to s_wave again puts a barrier of their own in between.

// the sum of v over the threads in front of this one; `total`: over all of them
template <int WAVES, class T>
__device__ __forceinline__ T block_prefix_excl(T v, uint32_t lane, uint32_t wid, T* s_wave) {
    const T incl = wave_prefix_incl(v, lane);
    if (lane == 63u) s_wave[wid] = incl;
    __syncthreads();
    T pre = incl - v;
    for (uint32_t w = 0; w < wid; ++w) pre += s_wave[w];
    return pre;
}
template <int WAVES, class T>
__device__ __forceinline__ T block_prefix_excl(T v, uint32_t lane, uint32_t wid, T* s_wave, T& total) {
    const T incl = wave_prefix_incl(v, lane);
    if (lane == 63u) s_wave[wid] = incl;
    __syncthreads();
    T pre = incl - v, all{};
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) { if (w < wid) pre += s_wave[w]; all += s_wave[w]; }
    total = all;
    return pre;
}

// the sum of v over the workgroup, in thread 0 (the others get what their wave's lanes hold: nothing to use)
template <int WAVES, class T>
__device__ __forceinline__ T block_sum(T v, T* s_wave) {
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    T all{};
    if (threadIdx.x == 0)
        for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) all += s_wave[w];
    return all;
}

// One workgroup of 1 024: out[i] = the sum of in[0 .. i), and done(the sum of all).  A lane owns four consecutive items per round,
// so a round covers 4 096 of them; the rounds in front are carried in LDS
template <class T, class Done>
__global__ __launch_bounds__(1024) void k_scan_items(const T* __restrict__ in, uint64_t n_items, T* __restrict__ out, Done done) {
    __shared__ T s_wave[16];
    __shared__ T s_carry;
    const uint32_t t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    if (t == 0) s_carry = T{};
    __syncthreads();
    for (uint64_t base = 0; base < n_items; base += 4096ull) {   // (uniform)
        const uint64_t i0 = base + (uint64_t)t * 4ull;
        T me[4], sum{}, all;
#pragma unroll
        for (int u = 0; u < 4; ++u) { me[u] = i0 + u < n_items ? in[i0 + u] : T{}; sum += me[u]; }
        T run = block_prefix_excl<16>(sum, lane, wid, s_wave, all);
        run += s_carry;
#pragma unroll
        for (int u = 0; u < 4; ++u) { if (i0 + u < n_items) out[i0 + u] = run; run += me[u]; }
        __syncthreads();
        if (t == 0) s_carry += all;
        __syncthreads();
    }
    if (t == 0) done(s_carry);
}

// the wave's words s[0 .. P) in LDS sorted ascending by a bitonic network; P a power of two >= 64, and what the lanes stored in
// front of the call is what is sorted.  (log2 P)(log2 P + 1) / 2 steps of P / 2 compare-exchanges, a lane taking every 64th
__device__ __forceinline__ void wave_sort_lds(uint32_t* s, uint32_t P, uint32_t lane) {
    wave_lds_sync();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t t = lane; t < P / 2u; t += 64u) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i + j;
                const uint32_t x = s[i], y = s[l];
                if ((x > y) == ((i & k) == 0u)) { s[i] = y; s[l] = x; }
            }
            wave_lds_sync();
        }
}

// the first place of the sorted words s[0 .. n) that holds v or more
__device__ __forceinline__ uint32_t lds_lower_bound(const uint32_t* s, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s[mid] < v) lo = mid + 1u; else hi = mid; }
    return lo;
}

// the threshold rule of classify (shared keys of a reference) and taxonomy (hit keys of a clade) for a record of `keys` keys
__device__ __forceinline__ bool passes_threshold(uint32_t shared, uint32_t keys, uint32_t min_keys, uint32_t num, uint32_t den) {
    return shared >= min_keys && (unsigned long long)shared * den >= (unsigned long long)num * keys;
}

// the long lists among the 64 a wave holds (a lane's: `len` holders from list[ls], is_long: more than the pass's cut), one after
// another by the whole wave: body(l, s0, n0) for the list of lane l, its start and its length in every lane
template <class Body>
__device__ __forceinline__ void wave_long_lists(bool is_long, uint32_t ls, uint32_t len, Body body) {
    unsigned long long left = __ballot(is_long);
    while (left) {
        const int l = __ffsll((long long)left) - 1;
        body(l, (uint32_t)__shfl(ls, l), (uint32_t)__shfl(len, l));
        left &= left - 1ull;
    }
}

// The route kernel of the two record calls, a lane per record: a record whose measure (classify: the work, the holders of its keys;
// taxonomy: its hit keys) is zero gets its row written here by empty(rec, r, keys); one of at most `cut` goes to the queue of the
// wave form, the others to the workgroup form's.  The queues' order is a race and no result depends on it
constexpr uint32_t kRouteThreads = 256;
enum { kRqSmall = 0, kRqLarge = 1, kRqBad = 2, kRqWords = 4 };   // words in front of the queues: their fill, the flag word, one spare
template <class Measure, class Empty>
__global__ __launch_bounds__(kRouteThreads) void k_rec_route(const uint64_t* __restrict__ off, uint32_t n_rec, const Measure* __restrict__ measure, Measure cut,
                                                             uint32_t* __restrict__ words, uint32_t* __restrict__ q_small, uint32_t* __restrict__ q_large,
                                                             uint4* __restrict__ rec, Empty empty) {
    const uint64_t r = (uint64_t)blockIdx.x * kRouteThreads + threadIdx.x;
    if (r >= n_rec) return;
    const Measure w = measure[r];
    if (w == 0) empty(rec, (uint32_t)r, (uint32_t)(off[r + 1] - off[r]));
    else if (w <= cut) q_small[atomicAdd(words + kRqSmall, 1u)] = (uint32_t)r;   // (a queue has room for every record)
    else q_large[atomicAdd(words + kRqLarge, 1u)] = (uint32_t)r;
}

// ---- What the two copies of records share (spsp_extract.hip: k_ex_copy, spsp_split.hip: k_sp_copy).

// 16 bytes at the 16-byte-aligned a < n: one load where they all lie in the text, the text's last bytes one by one
__device__ __forceinline__ uint4 ex_load16(const uint8_t* __restrict__ text, uint64_t n, uint64_t a) {
    if (a + 16 <= n) return *reinterpret_cast<const uint4*>(text + a);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j)
        if (a + j < n) w[j >> 2] |= (uint32_t)text[a + j] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the largest i of [lo, hi) with dst[i] <= o (dst[lo] <= o is the caller's)
__device__ __forceinline__ uint32_t ex_find(const uint64_t* __restrict__ dst, uint32_t lo, uint32_t hi, uint64_t o) {
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (dst[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// the 16 bytes of the text from s on (s + 15 < n), for an aligned store: the two aligned groups that hold them and a byte shift
__device__ __forceinline__ uint4 ex_gather16(const uint8_t* __restrict__ text, uint64_t n, uint64_t s) {
    const uint64_t a = s & ~15ull;
    uint32_t sh = (uint32_t)(s & 15ull);
    const uint4 lo4 = ex_load16(text, n, a);
    uint4 v;
    if (sh == 0u) v = lo4;
    else {
        const uint4 hi4 = ex_load16(text, n, a + 16ull);   // (holds byte s + 15, which is in the text)
        unsigned long long q0 = (unsigned long long)lo4.x | ((unsigned long long)lo4.y << 32), q1 = (unsigned long long)lo4.z | ((unsigned long long)lo4.w << 32);
        unsigned long long q2 = (unsigned long long)hi4.x | ((unsigned long long)hi4.y << 32);
        const unsigned long long q3 = (unsigned long long)hi4.z | ((unsigned long long)hi4.w << 32);
        if (sh >= 8u) { q0 = q1; q1 = q2; q2 = q3; sh -= 8u; }
        const uint32_t r = sh * 8u;
        const unsigned long long x0 = r ? (q0 >> r) | (q1 << (64u - r)) : q0, x1 = r ? (q1 >> r) | (q2 << (64u - r)) : q1;
        v = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32));
    }
    return v;
}

}  // namespace spsp
